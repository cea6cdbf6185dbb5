"""The colour augmentation of training frames (ImageTransformMulti(aug=True), transform.py:142-216):
thinktwice_amd.photometric (schedule, sampler, program compiler, apply_u8), TrainImagePipeline(augment=...) and the kernels
behind tt_photometric_u8 / tt_preprocess_images_ida_aug, against the numpy restatement tests/photometric_ref.py.

There is no golden from the reference here, and there cannot be one yet: the reference's augmenter is imgaug on top of cv2,
neither of which is installed where these tests were written, so no fixture of its arithmetic could be generated (SURVEY 8(c):
third-party bodies).  What is checked instead: the schedule against the literals of `augmenter()`, the laws of the sampler's
draws statistically (5 sigma bounds, worked out below from the binomial / uniform laws, so a correct sampler passes for any
seed), the conventions of the host functions by spot literals, and the device against the restatement BIT FOR BIT -- both
execute the same integer and f32 operations in the same order, so the expected number of differing bytes is zero."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import photometric_ref as R  # noqa: E402
from thinktwice_amd import calib, photometric as P  # noqa: E402
from thinktwice_amd.photometric import Program, Step  # noqa: E402


# ------------------------------------------------------------------------------------------------ CPU: schedule
def test_schedule_literals():
    s0, s1, s2 = (P.PhotometricSchedule(it) for it in (0, 270000, 1500000))
    assert [s.frequency for s in (s0, s1, s2)] == [0.05, 0.5, 1.0]
    assert [s.color for s in (s0, s1, s2)] == [0.0, 0.09, 0.5]
    assert s1.dropout == 0.06806042619907221
    assert abs(s0.dropout - 0.03856658) < 1e-15 and s0.blur == 0.5 and s1.blur == 0.95 and s2.blur == 1.0
    assert (s0.add, s0.mul_pos, s0.mul_neg, s0.con_pos, s0.con_neg) == (10, 1, 1, 1, 1)
    assert (s2.add, s2.mul_pos, s2.con_pos, s2.con_neg) == (60, 7.25, 1.5, 0.5)
    assert s2.mul_neg == 1 - 0.91 and abs(s2.mul_neg - 0.09) < 1e-15        # (0.08999999999999997 in the reference's own floats)
    assert max(P.PhotometricSchedule(it).dropout for it in (0, 10 ** 6, 10 ** 7, 10 ** 9)) < 0.198667 < P.MAX_NOISE_SCALE


# ------------------------------------------------------------------------------------------------ CPU: sampler
def test_same_seed_gives_identical_programs():
    a = P.PhotometricSampler(8, seed=11).programs(6, 37, 70, iteration=1500000)
    b = P.PhotometricSampler(8, seed=11).programs(6, 37, 70, iteration=1500000)
    c = P.PhotometricSampler(8, seed=12).programs(6, 37, 70, iteration=1500000)
    assert a == b and a != c
    assert P.PhotometricSampler(8, seed=np.random.RandomState(11)).programs(6, 37, 70, iteration=1500000) == a
    assert bytes(P.pack_programs(a).numpy()) == bytes(P.pack_programs(b).numpy())


def test_pinned_draw_of_seed_7():
    """The stream must not change by accident: the draw of RandomState(7) at iteration 270000, literally."""
    d = P.PhotometricSampler(8, seed=7).sample(1, iteration=270000)[0]
    assert d.iteration == 270000
    assert d.order == ("coarse", "multiply", "blur", "contrast", "dropout", "noise", "add", "gray")
    assert d.ops == (P.OpDraw("blur", False, (0.2550170310967776,), None),
                     P.OpDraw("contrast", False, (1.0546730264987876,), None),
                     P.OpDraw("dropout", True, (0.019611312296289127,), 16779039006144597436),
                     P.OpDraw("noise", False, (0.06337827857917645,), 459309668489100400))
    prog = P.compile_program(d, 37, 70)
    assert [s.kind for s in prog.steps] == [P.BLUR, P.LUT, P.DROPOUT, P.NOISE] and prog.blur_index == 0
    assert prog.steps[2].threshold == int(0.019611312296289127 * 2 ** 32) and prog.steps[2].per_channel
    assert prog.steps[3].cum == P.noise_thresholds(0.06337827857917645)


def test_read_counter_is_reads_over_batch_size():
    s = P.PhotometricSampler(4, seed=0, reads=6)
    its = [d.iteration for d in s.sample(5)]
    assert its == [1.5, 1.75, 2.0, 2.25, 2.5] and s.reads == 11
    assert [d.iteration for d in s.sample(2, iteration=99)] == [99, 99] and s.reads == 11
    with pytest.raises(ValueError):
        P.PhotometricSampler(0)


LIMITS = {"blur": lambda s: (0, s.blur), "noise": lambda s: (0, s.dropout), "dropout": lambda s: (0, s.dropout),
          "add": lambda s: (-s.add, s.add), "multiply": lambda s: (s.mul_neg, s.mul_pos), "contrast": lambda s: (s.con_neg, s.con_pos),
          "gray": lambda s: (0, 1)}


def _within_limits(d, s):
    for op in d.ops:
        if op.name == "coarse":
            assert 0 <= op.values[0] <= s.dropout and all(0.08 <= v <= 0.2 for v in op.values[1:]), op
        else:
            lo, hi = LIMITS[op.name](s)
            assert all(lo <= v <= hi for v in op.values), op
            assert len(op.values) == (3 if op.per_channel and op.name in ("add", "multiply", "contrast") else 1), op
        assert (op.seed is not None) == (op.name in ("noise", "dropout", "coarse")) and (op.seed is None or 0 <= op.seed < 2 ** 64)
        assert not (op.per_channel and op.name in ("blur", "gray"))


def test_laws_of_the_draws():
    """4000 samples.  At iteration 270000 (frequency 0.5): an operator's application count is Binomial(4000, 0.5), sigma =
    sqrt(4000 / 4) = 31.6, 5 sigma = 158; its position in the order is uniform on 0..7, variance 63 / 12, so the mean of 4000
    has sigma sqrt(5.25 / 4000) = 0.0362, 5 sigma = 0.181.  At iteration 1500000 (frequency 1, color 0.5): 6 x 4000 per-channel
    flags, share sigma sqrt(0.25 / 24000) = 0.00323, 5 sigma = 0.0161."""
    n = 4000
    draws = P.PhotometricSampler(8, seed=2024).sample(n, iteration=270000)
    s = P.PhotometricSchedule(270000)
    for name in P.OPERATORS:
        count = sum(any(op.name == name for op in d.ops) for d in draws)
        pos = np.mean([d.order.index(name) for d in draws])
        print(f"{name}: applied {count} of {n}, mean position {pos:.4f}")
        assert abs(count - n / 2) <= 158, (name, count)
        assert abs(pos - 3.5) <= 0.181, (name, pos)
    for d in draws:
        assert sorted(d.order) == sorted(P.OPERATORS)
        assert [op.name for op in d.ops] == [nm for nm in d.order if any(op.name == nm for op in d.ops)]      # execution order
        _within_limits(d, s)
    late = P.PhotometricSampler(8, seed=2025).sample(n, iteration=1500000)
    s = P.PhotometricSchedule(1500000)
    flags = [op.per_channel for d in late for op in d.ops if op.name not in ("blur", "gray")]
    assert len(flags) == 6 * n and all(len(d.ops) == 8 for d in late)
    print("per-channel share:", np.mean(flags))
    assert abs(np.mean(flags) - 0.5) <= 0.0161
    for d in late:
        _within_limits(d, s)
    early = P.PhotometricSampler(8, seed=2026).sample(n, iteration=0)
    assert not any(op.per_channel for d in early for op in d.ops)                                           # color = 0


# ------------------------------------------------------------------------------------------------ CPU: conventions
def test_lut_builders_spot_literals():
    assert P.add_lut(10.5).dtype == np.uint8 and (P.add_lut(10.5)[250:] == 255).all() and P.add_lut(10.5)[0] == 10      # rint(10.5) = 10
    assert list(P.add_lut(11.5)[:2]) == [12, 13]                                                                        # rint(11.5) = 12
    assert list(P.add_lut(-3.5)[0:5]) == [0, 0, 0, 0, 0] and P.add_lut(-3.5)[5] == 1                                    # k = -4
    assert list(P.multiply_lut(0.5)[:6]) == [0, 0, 1, 2, 2, 2] and P.multiply_lut(0.5)[255] == 128                      # ties to even
    assert P.multiply_lut(7.25)[36] == 255 and P.multiply_lut(7.25)[35] == 254
    assert list(P.contrast_lut(0.5)[[0, 126, 127, 128, 130, 255]]) == [64, 126, 127, 128, 128, 191]                     # 63.5 -> 64, 127.5 -> 128
    assert P.contrast_lut(1.5)[[0, 255]].tolist() == [0, 255] and (P.contrast_lut(1.0) == np.arange(256)).all()
    assert (P.add_lut(0.4) == np.arange(256)).all() and (P.multiply_lut(1.0) == np.arange(256)).all()


def test_adjacent_luts_compose_exactly():
    d = P.PhotometricDraw(0, P.OPERATORS, (P.OpDraw("add", True, (17.3, -40.2, 3.0), None),
                                           P.OpDraw("multiply", False, (1.7,), None),
                                           P.OpDraw("contrast", True, (0.6, 1.4, 1.0), None)))
    prog = P.compile_program(d, 8, 8)
    assert [s.kind for s in prog.steps] == [P.LUT]
    i = np.arange(256)
    for c, (a, k) in enumerate(zip((17.3, -40.2, 3.0), (0.6, 1.4, 1.0))):
        assert (prog.steps[0].lut[c] == P.contrast_lut(k)[P.multiply_lut(1.7)[P.add_lut(a)[i]]]).all(), c
    split = P.PhotometricDraw(0, P.OPERATORS, (d.ops[0], P.OpDraw("gray", False, (0.5,), None), d.ops[1]))
    assert [s.kind for s in P.compile_program(split, 8, 8).steps] == [P.LUT, P.GRAY, P.LUT]


def test_noise_thresholds():
    """k = +-1 each has probability Phi(-0.5 / 0.198667) = 5.922e-3 at the schedule's largest scale; over 2^22 field values
    the share has sigma sqrt(p (1 - p) / 2^22) = 3.75e-5, 5 sigma = 1.9e-4."""
    p1 = 0.5 * (1 + math.erf(-0.5 / 0.198667 / math.sqrt(2)))
    assert abs(p1 - 5.922e-3) < 1e-6
    u = R.field(987654321, 1 << 22)
    k = R.noise_k(u, P.noise_thresholds(0.198667))
    for v in (-1, 1):
        share = float(np.mean(k == v))
        print(f"k = {v}: share {share:.6e}")
        assert abs(share - 5.922e-3) <= 5 * math.sqrt(p1 * (1 - p1) / (1 << 22))
    assert set(np.unique(k)) <= {-1, 0, 1}
    assert (R.noise_k(u, P.noise_thresholds(0.0386)) == 0).all() and P.noise_is_zero(0.0386) and not P.noise_is_zero(0.198667)
    cum = P.noise_thresholds(0.5)
    assert list(cum) == sorted(cum) and cum[3] == int(2 ** 32 * 0.5 * (1 + math.erf(-1 / math.sqrt(2))))
    for bad in (0.51, 0.0, -1.0):
        with pytest.raises(ValueError):
            P.noise_thresholds(bad)
    with pytest.raises(ValueError):
        P.compile_program(P.PhotometricDraw(0, P.OPERATORS, (P.OpDraw("noise", False, (0.6,), 1),)), 8, 8)


def test_structures_mirror_the_header():
    import re
    from thinktwice_amd import _lib
    hdr = open(_lib.HEADER).read()
    assert int(re.search(r"#define TT_AUG_MAX_OPS (\d+)", hdr).group(1)) == P.TT_AUG_MAX_OPS == 8
    assert int(re.search(r"#define TT_AUG_NOISE_K (\d+)", hdr).group(1)) == P.TT_AUG_NOISE_K == 4
    for i, name in enumerate(P.KIND_NAMES):
        assert int(re.search(rf"#define TT_AUG_{name} (\d+)", hdr).group(1)) == i == getattr(P, name)
    assert ctypes.sizeof(P.AugOp) == 856 and ctypes.sizeof(P.AugProgram) == 6856          # static_assert'ed in csrc/photometric.hip
    assert P.AugOp.seed.offset == 24 and P.AugOp.cum.offset == 32 and P.AugOp.taps.offset == 64 and P.AugOp.lut.offset == 88
    assert P.AugProgram.ops.offset == 8
    L = _lib.lib()
    for n, h, w in ((64, 448, 896), (6, 37, 70), (1, 1, 1)):
        assert L.tt_photometric_scratch_bytes(n, h, w) == P.scratch_bytes(n, h, w) == n * h * w * 4
    assert L.tt_photometric_scratch_bytes(0, 5, 5) == 0 and L.tt_photometric_scratch_bytes(65535, 32768, 32768) == 65535 * 4 << 30


# ------------------------------------------------------------------------------------------------ CPU: restatement
def test_restatement_blur():
    for sigma in (1e-3, 0.3, 1.0):
        taps = P.blur_taps(sigma)
        assert abs(sum(taps) - 1) <= 1e-6 and taps[0] == taps[4] and taps[1] == taps[3] and all(t >= 0 for t in taps)
        for level in (0, 1, 77, 255):
            const = np.full((5, 7, 3), level, dtype=np.uint8)
            assert (R.apply_program(const, Program([Step(P.BLUR, taps=taps)], 5, 7)) == level).all(), (sigma, level)
    assert P.blur_taps(1e-3) == (0.0, 0.0, 1.0, 0.0, 0.0)
    img = np.zeros((6, 6, 3), dtype=np.uint8)
    img[0, 0] = 200                                        # a corner: reflect-101 mirrors its neighbours, not the corner itself
    t = [np.float32(x) for x in P.blur_taps(1.0)]
    out = R.apply_program(img, Program([Step(P.BLUR, taps=P.blur_taps(1.0))], 6, 6))
    assert out[0, 0, 0] == int(np.rint(t[2] * (t[2] * np.float32(200)))) and out[5, 5, 0] == 0
    assert out[2, 0, 0] == int(np.rint(t[0] * (t[2] * np.float32(200)))) and out[3, 0, 0] == 0
    for bad in (5e-4, 1.01):
        with pytest.raises(ValueError):
            P.blur_taps(bad)
    d = P.PhotometricDraw(0, P.OPERATORS, (P.OpDraw("blur", False, (5e-4,), None),))
    assert P.compile_program(d, 8, 8).steps == []           # sigma < 1e-3: dropped


def test_restatement_gray_is_the_identity_on_grey_images():
    assert 4899 + 9617 + 1868 == 1 << 14
    ramp = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    for alpha in (0.0, 0.123, 0.5, 0.999, 1.0):
        assert (R.apply_program(ramp, Program([Step(P.GRAY, alpha=P.gray_alpha(alpha))], 16, 16)) == ramp).all(), alpha
    red = np.zeros((1, 1, 3), dtype=np.uint8)
    red[..., 0] = 255
    assert R.apply_program(red, Program([Step(P.GRAY, alpha=1.0)], 1, 1)).tolist() == [[[76, 76, 76]]]        # (4899 * 255 + 8192) >> 14


def test_restatement_dropout_share():
    """37 x 70 elements at p = 0.15: sigma = sqrt(0.15 * 0.85 / 2590) = 7.02e-3, 5 sigma = 0.0351 (one field value per pixel);
    per channel 7770 elements: 5 sigma = 0.0203."""
    ones = np.full((37, 70, 3), 9, dtype=np.uint8)
    thr = P.dropout_threshold(0.15)
    assert thr == int(0.15 * 2 ** 32) and P.dropout_threshold(1.0) == 2 ** 32 - 1 and P.dropout_threshold(0.0) == 0
    shared = R.apply_program(ones, Program([Step(P.DROPOUT, False, threshold=thr, seed=12345)], 37, 70))
    assert ((shared == 0).all(axis=2) | (shared == 9).all(axis=2)).all()                     # the channels share the value
    per_ch = R.apply_program(ones, Program([Step(P.DROPOUT, True, threshold=thr, seed=12345)], 37, 70))
    a, b = float((shared[..., 0] == 0).mean()), float((per_ch == 0).mean())
    print(f"dropout share at seed 12345: shared {a:.4f}, per channel {b:.4f}")
    assert abs(a - 0.15) <= 0.0351 and abs(b - 0.15) <= 0.0203
    assert not ((per_ch == 0).all(axis=2) | (per_ch == 9).all(axis=2)).all()


def test_restatement_coarse_mask_is_constant_on_cells():
    assert P.coarse_grid(37, 70, 0.08, 0.2) == (3, 14) and int(37 * 0.08) == 2                # clamps to 3
    assert P.coarse_grid(448, 896, 0.2, 0.08) == (89, 71)
    for pc in (False, True):
        st = Step(P.COARSE, pc, grid=(3, 14), threshold=P.dropout_threshold(0.4), seed=77)
        m = R.coarse_mask(st, 37, 70)
        assert m.shape == (37, 70, 3) and 0 < m.mean() < 1
        cy, cx = np.arange(37) * 3 // 37, np.arange(70) * 14 // 70
        assert sorted(set(cy)) == [0, 1, 2] and sorted(set(cx)) == list(range(14))
        for i in range(3):
            for j in range(14):
                cell = m[cy == i][:, cx == j]
                assert (cell == cell[0, 0]).all()
        assert (m[..., 0] == m[..., 1]).all() != pc


# ------------------------------------------------------------------------------------------------ CPU: refusals
def _bad_programs():
    """(name, Program) the entries must refuse, for 37 x 70 images."""
    ok_lut = Step(P.LUT, lut=np.stack([P.add_lut(3)] * 3))
    taps = P.blur_taps(0.7)
    return [("too many steps", Program([ok_lut, Step(P.GRAY, alpha=0.5)] * 4 + [ok_lut], 37, 70)),
            ("unknown kind", Program([Step(6)], 37, 70)),
            ("two blurs", Program([Step(P.BLUR, taps=taps), ok_lut, Step(P.BLUR, taps=taps)], 37, 70)),
            ("negative tap", Program([Step(P.BLUR, taps=(-0.1, 0.3, 0.6, 0.3, -0.1))], 37, 70)),
            ("nan tap", Program([Step(P.BLUR, taps=(0.0, float("nan"), 1.0, 0.0, 0.0))], 37, 70)),
            ("taps do not sum to 1", Program([Step(P.BLUR, taps=(0.1, 0.2, 0.4, 0.2, 0.1001))], 37, 70)),
            ("grid of 0 rows", Program([Step(P.COARSE, False, grid=(0, 5), threshold=5, seed=1)], 37, 70)),
            ("grid wider than the image", Program([Step(P.COARSE, True, grid=(3, 71), threshold=5, seed=1)], 37, 70)),
            ("alpha above 1", Program([Step(P.GRAY, alpha=1.5)], 37, 70)),
            ("alpha nan", Program([Step(P.GRAY, alpha=float("nan"))], 37, 70)),
            ("decreasing thresholds", Program([Step(P.NOISE, False, seed=1, cum=(0, 0, 0, 9, 8, 10, 11, 12))], 37, 70))]


class _Recorder:
    def __init__(self, launched):
        self.launched = launched

    def __getattr__(self, name):
        return lambda *a: self.launched.append(name) or 0


def test_invalid_programs_raise_before_anything_is_launched(monkeypatch):
    from thinktwice_amd import preprocess
    from thinktwice_amd.preprocess import IdaParams
    launched = []
    monkeypatch.setattr(preprocess, "lib", lambda: _Recorder(launched))
    monkeypatch.setattr(P, "lib", lambda: _Recorder(launched))
    conf = dict(calib.IDA_AUG_CONF, final_dim=(37, 70))
    pipe = preprocess.TrainImagePipeline(conf, device="cpu", undistort=False)
    raw = torch.zeros(2, 1, 1, 900, 1600, 3, dtype=torch.uint8)
    params = [[IdaParams(0.1, 90, 160, 10, 10, False)]] * 2
    good = Program([], 37, 70)
    u8 = torch.zeros(2, 3, 37, 70, 3, dtype=torch.uint8)
    for name, bad in _bad_programs():
        with pytest.raises(ValueError, match="sample 1"):
            pipe(raw, params=params, augment=[good, bad])
        with pytest.raises(ValueError, match="sample 1"):
            P.apply_u8(u8, [good, bad])
    blur = Program([Step(P.BLUR, taps=P.blur_taps(0.7))], 2, 70)
    with pytest.raises(ValueError, match="sample 0"):
        P.apply_u8(torch.zeros(1, 1, 2, 70, 3, dtype=torch.uint8), [blur])                   # a blur needs H >= 3
    for wrong in ([good], [good, good, good], [good, None], [good, Program([], 38, 70)]):
        with pytest.raises(ValueError):
            pipe(raw, params=params, augment=wrong)
        with pytest.raises(ValueError):
            P.apply_u8(u8, wrong)
    for wrong in (u8.float(), u8[..., :2], u8[:, :, :, ::2], u8[0]):
        with pytest.raises(ValueError):
            P.apply_u8(wrong, [good, good])
    assert launched == []


def test_c_entries_refuse_invalid_programs_before_any_launch():
    """The C ABI's own check (host code only: every call here is refused before it touches the device)."""
    from thinktwice_amd import _lib
    from thinktwice_amd.preprocess import IdaSet
    L = _lib.lib()
    dummy = (ctypes.c_float * 4)(1, 1, 1, 1)                          # a non-null pointer no valid call would get this far with
    other = (ctypes.c_float * 4)(1, 1, 1, 1)
    sets = (IdaSet * 2)(IdaSet(90, 160, 10, 10, 0), IdaSet(90, 160, 10, 10, 1))
    good = Program([], 37, 70)

    def u8(host, dev=dummy, scratch=None, nbytes=0, H=37, W=70):
        return L.tt_photometric_u8(dummy, 2, 3, H, W, host, dev, scratch, nbytes, other, None)

    def fused(host, dev=dummy, scratch=None, nbytes=0, sets=sets, H=37, W=70):
        return L.tt_preprocess_images_ida_aug(dummy, 2, 2, 1, 900, 1600, dummy, dummy, sets, H, W, dummy, dummy, dummy, 4, 0, None,
                                              host, dev, scratch, nbytes, None)

    for name, bad in _bad_programs():
        host = (P.AugProgram * 2)(good.pack(), bad.pack())
        if name == "too many steps":
            host[1].num_ops = 9
        for call in (u8, fused):
            rc = call(host)
            assert rc == -1 and b"sample 1" in L.tt_last_error(), (name, call.__name__, rc, L.tt_last_error())
    host = (P.AugProgram * 2)(good.pack(), good.pack())
    host[1].blur_index = 0                                            # names a blur that is not there
    blurred = Program([Step(P.BLUR, taps=P.blur_taps(0.7))], 37, 70)
    need = 2 * 3 * 37 * 70 * 4
    for call in (u8, fused):
        assert call(host) == -1 and b"sample 1" in L.tt_last_error()
        assert call((P.AugProgram * 2)(good.pack(), good.pack()), dev=None) == -1 and b"device program" in L.tt_last_error()
        assert call(None) == -1
        with_blur = (P.AugProgram * 2)(good.pack(), blurred.pack())
        assert call(with_blur, scratch=None, nbytes=need) == -1 and b"scratch" in L.tt_last_error()
        assert call(with_blur, scratch=dummy, nbytes=(need if call is u8 else 2 * 2 * 37 * 70 * 4) - 1) == -1 and b"scratch" in L.tt_last_error()
        assert call(with_blur, scratch=dummy, nbytes=1 << 40, H=2) == -1 and b"sample 1" in L.tt_last_error()      # H >= 3
    assert L.tt_photometric_u8(dummy, 2, 3, 37, 70, (P.AugProgram * 2)(), dummy, None, 0, dummy, None) == -1      # out aliases in
    assert L.tt_photometric_u8(dummy, 0, 3, 37, 70, (P.AugProgram * 2)(), dummy, None, 0, other, None) == -1
    # the checks of tt_preprocess_images_ida, unchanged
    bad_sets = (IdaSet * 2)(IdaSet(90, 160, 10, 10, 0), IdaSet(90, 160, 54, 10, 0))
    assert fused((P.AugProgram * 2)(), sets=bad_sets) == -1 and b"set 1" in L.tt_last_error()
    assert fused((P.AugProgram * 2)(), sets=None) == -1


# ------------------------------------------------------------------------------------------------ GPU
def _images(seed, B, K, H, W):
    img = np.random.RandomState(seed).randint(0, 256, (B, K, H, W, 3)).astype(np.uint8)
    img[:, :, 0, 0] = 0
    img[:, :, 0, 1] = 255
    img[:, :, H - 1, W - 1] = (0, 255, 0)
    return img


def _differing_bytes(images, programs):
    got = P.apply_u8(torch.from_numpy(images).cuda(), programs).cpu().numpy()
    return int((got != R.apply_batch(images, programs)).sum()), got


def _single_step_programs(H, W):
    """{name: [program of sample 0, program of sample 1]}: every step kind alone, per-channel off and on."""
    lut_a, lut_b = np.stack([P.multiply_lut(1.7)] * 3), np.stack([P.add_lut(-40), P.contrast_lut(0.5), P.multiply_lut(7.25)])
    out = {"lut": [[Step(P.LUT, lut=lut_a)], [Step(P.LUT, lut=lut_b)]],
           "gray": [[Step(P.GRAY, alpha=P.gray_alpha(0.37))], [Step(P.GRAY, alpha=1.0)]],
           "blur": [[Step(P.BLUR, taps=P.blur_taps(1.0))], [Step(P.BLUR, taps=P.blur_taps(0.45))]],
           "blur and none": [[Step(P.BLUR, taps=P.blur_taps(0.8))], []]}
    for pc in (False, True):
        out[f"noise pc={pc}"] = [[Step(P.NOISE, pc, seed=2 ** 63 + 5, cum=P.noise_thresholds(0.198667))],
                                 [Step(P.NOISE, pc, seed=6, cum=P.noise_thresholds(0.5))]]
        out[f"dropout pc={pc}"] = [[Step(P.DROPOUT, pc, threshold=P.dropout_threshold(0.15), seed=2 ** 64 - 1)],
                                   [Step(P.DROPOUT, pc, threshold=P.dropout_threshold(0.5), seed=0)]]
        out[f"coarse pc={pc}"] = [[Step(P.COARSE, pc, grid=P.coarse_grid(H, W, 0.08, 0.2), threshold=P.dropout_threshold(0.3), seed=9)],
                                  [Step(P.COARSE, pc, grid=(H, W), threshold=P.dropout_threshold(0.5), seed=10)]]
    return {k: [Program(s, H, W) for s in v] for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(5, 7), (37, 70), (64, 128), (130, 67)])
def test_every_step_kind_alone_is_bit_equal_to_the_restatement(hw):
    H, W = hw
    images = _images(H * 1000 + W, 2, 3, H, W)
    assert images.min() == 0 and images.max() == 255
    for name, programs in _single_step_programs(H, W).items():
        diff, got = _differing_bytes(images, programs)
        print(f"{H} x {W} {name}: {diff} differing bytes of {images.size}")
        assert diff == 0, (hw, name, diff)
        if name != "blur and none":
            assert (got != images).any(), (hw, name)
        else:
            assert (got[1] == images[1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("iteration", [1500000, 270000])
def test_sampler_programs_are_bit_equal_to_the_restatement(iteration):
    H, W = 37, 70
    draws = [P.PhotometricSampler(8, seed=s).sample(1, iteration=iteration)[0] for s in range(6)]
    programs = [P.compile_program(d, H, W) for d in draws]
    if iteration == 1500000:                                          # all eight operators; the blur somewhere in mid-sequence
        assert all(len(d.ops) == 8 for d in draws)
        assert any(0 < p.blur_index < len(p) - 1 for p in programs)
    images = _images(iteration, 6, 3, H, W)
    diff, got = _differing_bytes(images, programs)
    print(f"iteration {iteration}: {[repr(p) for p in programs]}: {diff} differing bytes of {images.size}")
    assert diff == 0


@pytest.mark.gpu
def test_frames_of_a_sample_share_the_program_and_the_fields():
    H, W = 37, 70
    one = _images(5, 1, 1, H, W)
    images = np.ascontiguousarray(np.broadcast_to(one, (2, 3, H, W, 3)))
    programs = [P.PhotometricSampler(8, seed=s).programs(1, H, W, iteration=1500000)[0] for s in (1, 2)]
    got = P.apply_u8(torch.from_numpy(images).cuda(), programs).cpu().numpy()
    for b in range(2):
        assert (got[b] == got[b, :1]).all(), b
    assert (got[0] != got[1]).any() and programs[0] != programs[1]
    again = P.apply_u8(torch.from_numpy(images).cuda(), programs).cpu().numpy()
    assert (again == got).all()


HW = (128, 256)
MEAN = np.asarray(calib.IMAGENET_MEAN, dtype=np.float32).reshape(1, 1, 1, 3, 1, 1)
STD = np.asarray(calib.IMAGENET_STD, dtype=np.float32).reshape(1, 1, 1, 3, 1, 1)


@functools.lru_cache(maxsize=None)
def _fused():
    """One set of pipeline runs on raw 900 x 1600 synthetic frames (B = 2, final_dim 128 x 256), shared by the tests below."""
    from thinktwice_amd import synth
    from thinktwice_amd.preprocess import IdaSampler, TrainImagePipeline
    conf = dict(calib.IDA_AUG_CONF, final_dim=HW, resize_lim=(0.16, 0.18))
    raw = torch.stack([torch.from_numpy(synth.raw_camera_frames(s)) for s in (18, 19)]).cuda()
    lab = [synth.raw_label_maps(s) for s in (18, 19)]
    depth, seg = (torch.stack([torch.from_numpy(x[i]) for x in lab]).cuda() for i in range(2))
    pipe = TrainImagePipeline(conf)
    params = IdaSampler(conf, seed=3).sample(2, 4)
    empty = [Program([], *HW), Program([], *HW)]
    programs = P.PhotometricSampler(2, seed=4).programs(2, *HW, iteration=1500000)
    assert all(p.blur_index >= 0 and len(p) >= 4 for p in programs)
    run = lambda **kw: pipe(raw, depth, seg, params=params, **kw)      # noqa: E731
    return dict(pipe=pipe, run=run, programs=programs, plain=run(), empty=run(augment=empty), aug=run(augment=programs))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
def test_fused_entry_equals_truncation_then_apply_u8_then_normalisation():
    f = _fused()
    base = f["empty"]["img"].cpu().numpy().astype(np.float64)                       # [B, T, N, 3, h, w]
    level = (base * STD + MEAN) * 255
    grey = np.rint(level)
    assert np.abs(level - grey).max() < 1e-2 and grey.min() >= 0 and grey.max() <= 255
    u8 = np.ascontiguousarray(grey.astype(np.uint8).reshape(2, 8, 3, *HW).transpose(0, 1, 3, 4, 2))
    out = P.apply_u8(torch.from_numpy(u8).cuda(), f["programs"]).cpu().numpy()
    assert (out != u8).any()
    out = out.transpose(0, 1, 4, 2, 3).reshape(2, 2, 4, 3, *HW).astype(np.float32)
    expect = (out / np.float32(255) - MEAN) * (np.float32(1) / STD)
    assert expect.dtype == np.float32
    got = f["aug"]["img"].cpu().numpy()
    diff = int((got.view(np.int32) != expect.view(np.int32)).sum())
    print(f"fused vs two-step: {diff} differing values of {got.size}")
    assert diff == 0
    assert f["aug"]["programs"] == f["programs"] and "programs" not in f["plain"]


@pytest.mark.gpu
def test_fused_output_forms_agree():
    from thinktwice_amd import ops
    f = _fused()
    nchw = f["aug"]["img"].view(16, 3, *HW)
    cl = f["run"](augment=f["programs"], channel_last_dtype=torch.float32)["img"]
    assert cl.shape == (16, *HW, 4) and float(cl[..., 3].abs().max()) == 0.0
    assert torch.equal(_bits(cl[..., :3].permute(0, 3, 1, 2)), _bits(nchw))
    for dt in (torch.bfloat16, torch.float16):
        got = f["run"](augment=f["programs"], channel_last_dtype=dt)["img"]
        assert got.shape == (16, *HW, 8) and got.dtype == dt
        assert torch.equal(got.view(torch.int16), ops.nchw_to_nhwc_pad(nchw, dt, 8).view(torch.int16))
    cl6 = f["run"](augment=f["programs"], channel_last_dtype=torch.float32, c_pad=6)["img"]
    assert torch.equal(_bits(cl6[..., :3]), _bits(cl[..., :3])) and float(cl6[..., 3:].abs().max()) == 0.0


@pytest.mark.gpu
def test_empty_programs_differ_from_the_plain_pipeline_by_the_uint8_truncation():
    f = _fused()
    level = (f["plain"]["img"].cpu().numpy().astype(np.float64) * STD + MEAN) * 255
    grey = np.rint((f["empty"]["img"].cpu().numpy().astype(np.float64) * STD + MEAN) * 255)
    d = grey - level
    print(f"grey level - untruncated level: min {d.min():.6f} max {d.max():.6f}")
    assert d.min() > -1 - 1e-3 and d.max() <= 1e-3
    assert d.mean() < -0.3                                             # (a truncation, not a rounding)


@pytest.mark.gpu
def test_labels_and_ida_mats_are_untouched_and_calls_repeat_bit_for_bit():
    f = _fused()
    for k in ("depth", "seg"):
        assert torch.equal(_bits(f["plain"][k]), _bits(f["aug"][k])) and torch.equal(_bits(f["plain"][k]), _bits(f["empty"][k])), k
    assert torch.equal(f["plain"]["ida_mats"], f["aug"]["ida_mats"]) and f["plain"]["params"] == f["aug"]["params"]
    again = f["run"](augment=f["programs"])
    assert torch.equal(_bits(again["img"]), _bits(f["aug"]["img"]))
    assert not torch.equal(f["aug"]["img"], f["empty"]["img"])
    from thinktwice_amd.photometric import PhotometricSampler
    a = f["run"](augment=PhotometricSampler(2, seed=4, reads=3000000))
    b = f["run"](augment=PhotometricSampler(2, seed=4, reads=3000000))
    assert a["programs"] == b["programs"] and torch.equal(_bits(a["img"]), _bits(b["img"]))
