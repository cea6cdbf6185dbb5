"""csrc/eval_metrics.hip on the GPU, every entry against its numpy restatement (tests/eval_ref.py).  Integers are equal, not
close; the f64 L1 sums are bit-equal (subtract, absolute value, add in the stated order); the L2 sums carry a square root and
are compared with the relative limit recorded in profiles/eval_metrics.txt."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eval_ref as E  # noqa: E402

pytestmark = pytest.mark.gpu
D_BOUND = (1.0, 41.0, 0.5)                       # thinktwice_amd/config.py (CFG:136): the model's d_bound
SENTINEL = -0x0123456789ABCDEF
# profiles/eval_metrics.txt: the worst relative error of an L2 sum against the restatement observed on the GPU is 0 -- the f64
# square root is correctly rounded on both sides and every other step is one IEEE operation in the stated order -- so the limit,
# 4 x the worst observed, is 0 as well: the L2 sums are held to the restatement's bits like the L1 sums.
L2_REL_LIMIT = 4 * 0.0


def _lib():
    from thinktwice_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n, dtype=torch.int64):
    """n zeroed slots between two sentinel rows of 8."""
    buf = torch.full((n + 16,), SENTINEL, dtype=torch.int64, device="cuda")
    buf[8:8 + n] = 0
    return buf, (buf[8:8 + n] if dtype == torch.int64 else buf[8:8 + n].view(dtype))


def _untouched(buf, n):
    host = buf.cpu()
    return bool((host[:8] == SENTINEL).all() and (host[8 + n:] == SENTINEL).all())


@pytest.fixture(scope="module")
def seg_case():
    rng = np.random.default_rng(0)
    BN, h, w, f, cs, C = 3, 5, 7, 2, 16, 12
    logits = rng.standard_normal((BN, h, w, cs)).astype(np.float32)
    logits[..., C:] = rng.standard_normal((BN, h, w, cs - C)).astype(np.float32) * 4
    labels = rng.integers(0, C, (BN, h * f, w * f)).astype(np.float32)
    labels[:, 1::2, :] = 7                                           # pixels no cell reads
    logits[0, 0, 0, :C] = -1.0
    logits[0, 0, 0, [3, 9]] = 2.5                                    # a tie between two classes: the lower one
    logits[0, 0, 1, :C] = 0.0
    logits[0, 0, 1, [5, 11]] = 1.0
    logits[0, 0, 1, 13] = 1.0                                        # a tie with a padding channel...
    logits[0, 0, 1, 12] = 50.0                                       # ...and a padding channel holding a larger value
    logits[0, 0, 2, 4] = np.nan                                      # a NaN among the classes
    logits[0, 0, 3, 14] = np.nan                                     # a NaN in the padding: not read
    labels[0, 0, 2 * 4] = 255                                        # ignored ...
    logits[0, 0, 4, 0] = np.nan                                      # ... whatever its logits hold
    labels[0, 0, 2 * 5] = 12                                         # out of range
    labels[1, 2, 2 * 3] = -3
    want = E.seg_confusion(logits, labels, C, f)
    assert want[1] == 2 and want[2] == 1 and want[0][labels[0, 0, 0].astype(int), 3] >= 1 and want[0][:, 5].sum() >= 1
    return dict(logits=logits, labels=labels, dims=(BN, h * f, w * f, f, cs, C), want=want)


def _seg(case, conf, logits=None, cstride=None):
    BN, H, W, f, cs, C = case["dims"]
    lg = torch.from_numpy(case["logits"] if logits is None else logits).cuda()
    lb = torch.from_numpy(case["labels"]).cuda()
    L = _lib()
    L.check(L.lib().tt_eval_seg_confusion(L.ptr(lg), cstride or cs, C, L.ptr(lb), BN, H, W, f, L.ptr(conf), _stream()),
            "tt_eval_seg_confusion")
    torch.cuda.synchronize()


def test_seg_confusion_equals_the_restatement_and_accumulates(seg_case):
    C = seg_case["dims"][-1]
    conf_w, bad_w, nf_w = seg_case["want"]
    want = np.concatenate([conf_w.reshape(-1), [bad_w, nf_w]]).astype(np.int64)
    buf, conf = _guarded(C * C + 2)
    _seg(seg_case, conf)
    first = conf.cpu().numpy().copy()
    assert np.array_equal(first, want)
    assert first.sum() == 3 * 5 * 7 - 1                              # every cell but the ignored one, once
    buf2, conf2 = _guarded(C * C + 2)
    _seg(seg_case, conf2)
    assert torch.equal(conf2, torch.from_numpy(first).cuda())        # two runs: the same bits
    _seg(seg_case, conf)                                             # a second add accumulates into the first
    assert np.array_equal(conf.cpu().numpy(), 2 * want)
    assert _untouched(buf, C * C + 2) and _untouched(buf2, C * C + 2)


def test_seg_confusion_scalar_form_reads_a_pitch_that_is_no_multiple_of_four(seg_case):
    BN, H, W, f, cs, C = seg_case["dims"]
    logits = np.ascontiguousarray(seg_case["logits"][..., :13])      # pitch 13: the one-lane-per-cell form
    want = E.seg_confusion(logits, seg_case["labels"], C, f)
    buf, conf = _guarded(C * C + 2)
    _seg(seg_case, conf, logits=logits, cstride=13)
    assert np.array_equal(conf.cpu().numpy(), np.concatenate([want[0].reshape(-1), [want[1], want[2]]]))
    assert _untouched(buf, C * C + 2)


def test_seg_confusion_over_more_than_one_workgroup():
    rng = np.random.default_rng(5)
    BN, H, W, f, cs, C = 2, 70, 66, 2, 16, 12                        # 2310 cells at 64 per workgroup
    logits = rng.standard_normal((BN, H // f, W // f, cs)).astype(np.float32)
    labels = rng.integers(0, C + 1, (BN, H, W)).astype(np.float32)
    labels[labels == C] = 255
    want = E.seg_confusion(logits, labels, C, f)
    buf, conf = _guarded(C * C + 2)
    L = _lib()
    lg, lb = torch.from_numpy(logits).cuda(), torch.from_numpy(labels).cuda()
    L.check(L.lib().tt_eval_seg_confusion(L.ptr(lg), cs, C, L.ptr(lb), BN, H, W, f, L.ptr(conf), _stream()), "seg")
    assert np.array_equal(conf.cpu().numpy(), np.concatenate([want[0].reshape(-1), [want[1], want[2]]]))
    assert _untouched(buf, C * C + 2)


@pytest.mark.parametrize("cstride", [80, 81])
def test_depth_bins_equal_the_restatement(cstride):
    rng = np.random.default_rng(1)
    BN, H, W, f = 2, 32, 48, 16
    D = int((D_BOUND[1] - D_BOUND[0]) / D_BOUND[2])
    h, w = H // f, W // f
    gt = np.zeros((BN, H, W), np.float32)
    mask = rng.random(gt.shape) < 0.02
    gt[mask] = rng.uniform(0.3, 44.0, int(mask.sum())).astype(np.float32)
    cells = gt.reshape(BN, h, f, w, f)
    cells[0, 0, :, 0, :] = 0.0                                       # background
    cells[0, 0, :, 1, :] = 0.0
    cells[0, 0, 15, 1, 15] = 1.0                                     # on the first edge
    cells[0, 1, :, 0, :] = 0.0
    cells[0, 1, 3, 0, 2] = 41.0                                      # D + 1: out of range
    cells[1, 1, :, 2, :] = 0.0
    cells[1, 1, 0, 2, 0] = 20.0
    logits = rng.standard_normal((BN, h, w, cstride)).astype(np.float32)
    bins = E.depth_cell_bins(gt, f, D_BOUND[0], D_BOUND[2], D)
    assert bins[0, 0, 0] == 0 and bins[0, 0, 1] == 1 and bins[0, 1, 0] == 0 and bins[1, 1, 2] == 39
    logits[0, 0, 1, :D] = 0.0
    logits[0, 0, 1, [0, 40]] = 3.0                                   # a tie: the lower channel, which is the bin's
    logits[1, 1, 2, 17] = np.nan                                     # a foreground cell with a NaN
    logits[0, 1, 0, 5] = np.nan                                      # a background cell: not read
    for y in range(h):                                               # make top-1, within-1 and far misses all occur
        for x in range(w):
            if bins[1, y, x] >= 1 and (y, x) != (1, 2):
                logits[1, y, x, min(D - 1, bins[1, y, x] - 1 + (x % 3))] = 9.0
    if cstride > D:
        logits[..., D:] = 99.0                                       # padding: takes no part
    want = E.depth_bins(logits, gt, D, f, D_BOUND[0], D_BOUND[2])
    assert want[4] == 1 and want[0] > want[1] > 0 and want[2] > want[1] and want[3] > want[2] - want[1]
    buf, acc = _guarded(5)
    L = _lib()
    lg, g = torch.from_numpy(logits).cuda(), torch.from_numpy(gt).cuda()
    for rep in (1, 2):
        L.check(L.lib().tt_eval_depth_bins(L.ptr(lg), cstride, D, L.ptr(g), BN, H, W, f, D_BOUND[0], D_BOUND[2], L.ptr(acc),
                                           _stream()), "tt_eval_depth_bins")
        assert acc.cpu().tolist() == [rep * v for v in want]
    assert _untouched(buf, 5)


def _decoder_inputs(rng, B, S):
    f = lambda *s: rng.standard_normal(s).astype(np.float32)                                           # noqa: E731
    return dict(pred_wp=f(B, S, 4, 2) * 5, mu=f(B, S, 2), sigma=np.abs(f(B, S, 2)) + 0.1, pred_speed=np.abs(f(B, 1)) * 0.5,
                wp=f(B, 4, 2) * 5, a_mu=f(B, 2), a_sigma=np.abs(f(B, 2)) + 0.1, speed=np.abs(f(B)) * 6)


def _run_decoder(x, sums, counts):
    L = _lib()
    t = {k: torch.from_numpy(v).cuda() for k, v in x.items()}
    B, S = x["pred_wp"].shape[:2]
    L.check(L.lib().tt_eval_decoder(L.ptr(t["pred_wp"]), L.ptr(t["mu"]), L.ptr(t["sigma"]), L.ptr(t["pred_speed"]), L.ptr(t["wp"]),
                                    L.ptr(t["a_mu"]), L.ptr(t["a_sigma"]), L.ptr(t["speed"]), B, S, L.ptr(sums), L.ptr(counts),
                                    _stream()), "tt_eval_decoder")
    torch.cuda.synchronize()


def test_decoder_sums_equal_the_restatement():
    rng = np.random.default_rng(2)
    B, S = 3, 6
    n = 8 * S + 1
    buf, sums = _guarded(n, torch.float64)
    cbuf, counts = _guarded(2)
    want_s, want_c = None, None
    worst = 0.0
    for rep in range(2):                                             # the second call goes on with the first one's sums
        x = _decoder_inputs(rng, B, S)
        if rep == 1:
            x["pred_wp"][1, 4, 2, 0] = np.nan                        # a sample with a NaN waypoint: nonfinite only
        _run_decoder(x, sums, counts)
        want_s, want_c = E.decoder(**x, sums=want_s, counts=want_c)
        got = sums.cpu().numpy()
        l1 = [i for i in range(n) if i == 8 * S or i % 8 >= 2]
        l2 = [i for i in range(n) if i != 8 * S and i % 8 < 2]
        assert np.array_equal(got[l1].view(np.int64), want_s[l1].view(np.int64)), (got[l1], want_s[l1])
        rel = np.abs(got[l2] - want_s[l2]) / np.abs(want_s[l2])
        worst = max(worst, float(rel.max()))
        print(f"tt_eval_decoder L2 sums, call {rep}: worst relative error {rel.max():.3e} (limit {L2_REL_LIMIT:.3e})")
        assert rel.max() <= L2_REL_LIMIT
        assert counts.cpu().tolist() == want_c
    assert want_c == [5, 1] and np.isfinite(sums.cpu().numpy()).all()
    assert _untouched(buf, n) and _untouched(cbuf, 2)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_pair_deviation_against_itself_and_a_known_pair(n):
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n).astype(np.float32)
    L = _lib()
    ta = torch.from_numpy(a).cuda()
    buf, slots = _guarded(3)
    L.check(L.lib().tt_eval_pair_deviation(L.ptr(ta), L.ptr(ta), n, L.ptr(slots), _stream()), "pair")
    bits = slots.cpu().tolist()
    assert bits == [0, int(np.abs(a).max().view(np.uint32)), 0]      # 0, its max, 0
    b = a.copy()
    k = n - 1
    a[k], b[k] = 7.0, 7.0 - 2.5                                      # the known maximum, in the last element
    if n > 2:
        b[0] = np.inf                                                # stays out of both maxima
        a[1], b[1] = np.nan, 100.0
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    slots.zero_()
    want = E.pair_deviation(a, b)
    for rep in range(2):                                             # folding the same pair again changes nothing but the count
        L.check(L.lib().tt_eval_pair_deviation(L.ptr(ta), L.ptr(tb), n, L.ptr(slots), _stream()), "pair")
        got = slots.cpu().tolist()
        assert got == [int(want[0].view(np.uint32)), int(want[1].view(np.uint32)), (rep + 1) * want[2]]
    assert want[0] == np.float32(2.5) and want[1] == np.float32(7.0) and want[2] == (2 if n > 2 else 0)
    # an unaligned view takes the scalar form
    if n > 4:
        L.check(L.lib().tt_eval_pair_deviation(L.ptr(ta[1:]), L.ptr(tb[1:]), n - 1, L.ptr(slots), _stream()), "pair")
        assert slots.cpu().tolist()[:2] == got[:2]
    assert _untouched(buf, 3)


def test_pair_wp_and_pair_seg_equal_the_restatement(seg_case):
    rng = np.random.default_rng(3)
    L = _lib()
    a = rng.standard_normal((3, 6, 4, 2)).astype(np.float32)
    b = (a + rng.standard_normal(a.shape).astype(np.float32) * 1e-3).astype(np.float32)
    b[2, 5, 3, 1] = np.inf
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    buf, ms = _guarded(2, torch.float64)
    cbuf, counts = _guarded(2)
    want_ms, want_c = (0.0, 0.0), (0, 0)
    for rep in range(2):
        L.check(L.lib().tt_eval_pair_wp(L.ptr(ta), L.ptr(tb), a.size // 2, L.ptr(ms), L.ptr(counts), _stream()), "pair_wp")
        want_ms, want_c = E.pair_wp(a, b, want_ms, want_c)
        got = ms.cpu().tolist()
        assert got[0] == want_ms[0] and abs(got[1] - want_ms[1]) <= L2_REL_LIMIT * want_ms[1], (got, want_ms)
        assert counts.cpu().tolist() == want_c
    assert want_c == [2 * 71, 2] and _untouched(buf, 2) and _untouched(cbuf, 2)
    L.check(L.lib().tt_eval_pair_wp(L.ptr(ta), L.ptr(ta), a.size // 2, L.ptr(ms.zero_()), L.ptr(counts.zero_()), _stream()), "pair_wp")
    assert ms.cpu().tolist() == [0.0, 0.0] and counts.cpu().tolist() == [72, 0]
    # seg maps: the hand-made cells of the confusion case against a copy with three changed cells
    BN, H, W, f, cs, C = seg_case["dims"]
    sa = seg_case["logits"]
    sb = sa.copy()
    sb[1, 1, 1, :C] = 0.0
    sb[1, 1, 1, (int(np.argmax(sa[1, 1, 1, :C])) + 1) % C] = 1.0     # another class
    sb[2, 4, 6, 12:] = 1e3                                           # padding only: the same class
    sb[2, 0, 0, :C] += 1.0                                           # shifted: the same class
    want = E.pair_seg(sa, sb, C)
    assert want == [1, BN * 5 * 7 - 2, 2]
    obuf, out = _guarded(3)
    tsa, tsb = torch.from_numpy(sa).cuda(), torch.from_numpy(sb).cuda()
    L.check(L.lib().tt_eval_pair_seg(L.ptr(tsa), L.ptr(tsb), cs, C, BN * 5 * 7, L.ptr(out), _stream()), "pair_seg")
    assert out.cpu().tolist() == want
    L.check(L.lib().tt_eval_pair_seg(L.ptr(tsa), L.ptr(tsa), cs, C, BN * 5 * 7, L.ptr(out.zero_()), _stream()), "pair_seg")
    assert out.cpu().tolist() == [0, want[1], 2] and _untouched(obuf, 3)


def test_the_host_rejects_bad_arguments():
    L = _lib()
    lib = L.lib()
    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    acc = torch.zeros(256, dtype=torch.int64, device="cuda")
    p, a, st = L.ptr(x), L.ptr(acc), _stream()

    def err():
        return lib.tt_last_error().decode()
    assert lib.tt_eval_seg_confusion(None, 16, 12, p, 1, 2, 2, 2, a, st) == -1 and "null" in err()
    assert lib.tt_eval_seg_confusion(p, 16, 12, p, 1, 2, 2, 2, None, st) == -1 and "null" in err()
    assert lib.tt_eval_seg_confusion(p, 8, 12, p, 1, 2, 2, 2, a, st) == -1 and "cstride" in err()
    assert lib.tt_eval_seg_confusion(p, 16, 12, p, 1, 3, 2, 2, a, st) == -1 and "divisible" in err()
    assert lib.tt_eval_seg_confusion(p, 16, 12, p, 1, 2, 3, 2, a, st) == -1 and "divisible" in err()
    assert lib.tt_eval_seg_confusion(p, 64, 33, p, 1, 2, 2, 2, a, st) == -1 and "num_classes" in err()
    assert lib.tt_eval_depth_bins(p, 80, 80, None, 1, 16, 16, 16, 1.0, 0.5, a, st) == -1 and "null" in err()
    assert lib.tt_eval_depth_bins(p, 64, 80, p, 1, 16, 16, 16, 1.0, 0.5, a, st) == -1 and "cstride" in err()
    assert lib.tt_eval_depth_bins(p, 80, 80, p, 1, 16, 24, 16, 1.0, 0.5, a, st) == -1 and "divisible" in err()
    assert lib.tt_eval_decoder(p, p, p, p, p, p, p, None, 1, 6, a, a, st) == -1 and "null" in err()
    assert lib.tt_eval_decoder(p, p, p, p, p, p, p, p, 1, 8, a, a, st) == -1 and "S 8" in err()
    assert lib.tt_eval_pair_deviation(p, None, 4, a, st) == -1 and "null" in err()
    assert lib.tt_eval_pair_deviation(p, p, 0, a, st) == -1
    assert lib.tt_eval_pair_wp(p, p, 0, a, a, st) == -1 and lib.tt_eval_pair_wp(None, p, 1, a, a, st) == -1
    assert lib.tt_eval_pair_seg(p, p, 8, 12, 1, a, st) == -1 and "cstride" in err()
    torch.cuda.synchronize()
    assert int(acc.sum()) == 0                                       # nothing was launched
