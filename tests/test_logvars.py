"""Device log windows (csrc/logvars.hip, thinktwice_amd/logvars.py) against the torch expression of losses.parse_losses and the
host restatements of tests/logvars_ref.py: every comparison is of bits."""
import ctypes
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import logvars_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
HW, B, NPTS = (128, 256), 2, 4096


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).tolist()


def _bits_of_floats(values):
    return np.asarray(values, dtype=np.float32).view(np.int32).tolist()


@pytest.fixture(scope="module")
def real():
    """One forward_train of the test_train_step setup: (model, its dict of loss terms)."""
    from thinktwice_amd import model as tm, params, synth
    m, cfg = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    m.load_state_dict(params.init_params(cfg, seed=0))
    batch = synth.make_batch(B, img_hw=HW, num_points=NPTS)
    batch.update(synth.make_train_targets(B, img_hw=HW))
    losses = m.forward_train(batch)
    torch.cuda.synchronize()
    return m, losses


def _t(v):
    return torch.tensor(v, dtype=torch.float32, device="cuda")


def _spread(rng, k):
    return [float(np.float32(rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-6, 6))) for _ in range(k)]


def _cases():
    rng = np.random.default_rng(11)
    nan = float("nan")
    v = _spread(rng, 64)
    w = _spread(rng, 64)
    return {
        "one term": OrderedDict(a_loss=1.5),
        "64 terms, one per name": OrderedDict((f"t{i}_loss" if i % 3 else f"t{i}_offset", v[i]) for i in range(64)),
        "64 terms in lists": OrderedDict(a_loss=w[:32], b_offset=w[32:63], c_loss=w[63]),
        "a list of 3": OrderedDict(a_loss=[0.1, 0.2, 0.3], b=4.0, c_loss=1e-8, d_loss=[1e8, -1e8, 1.0]),
        "-0.0": OrderedDict(a_loss=-0.0, b=-0.0, c_loss=[-0.0], d=[-0.0, -0.0]),
        "only -0.0 in the total": OrderedDict(a_loss=-0.0),
        "NaN": OrderedDict(a_loss=nan, b_loss=1.0, c=[nan, 2.0], d=3.0),
        "a NaN that is not logged as loss": OrderedDict(a=nan, b_loss=1.0),
    }


@pytest.mark.parametrize("case", list(_cases()))
def test_pack_is_the_torch_expression_bit_for_bit(case):
    from thinktwice_amd import logvars, losses as LS
    spec = _cases()[case]
    dev = OrderedDict((k, [_t(x) for x in v] if isinstance(v, list) else _t(v)) for k, v in spec.items())
    loss0, floats = LS.parse_losses(dev)
    names, packed, loss = logvars.pack(dev)
    assert names == tuple(floats) == tuple(spec) + ("loss",)
    assert packed.dtype == torch.float32 and packed.shape == (len(spec) + 1,)
    got = _bits(packed)
    assert got == _bits_of_floats(list(floats.values())), (case, packed.tolist(), list(floats.values()))
    assert _bits(loss.reshape(1)) == _bits(loss0.reshape(1)) == got[-1:]
    assert loss.data_ptr() == packed.data_ptr() + 4 * len(spec)          # a view of the same vector
    ref_names, ref = R.pack_ref(spec)
    assert ref_names == names and got == _bits_of_floats(ref)
    loss1, dlv = LS.parse_losses(dev, device_log=True)
    assert isinstance(dlv, logvars.DeviceLogVars) and dlv.names == names and _bits(dlv.packed) == got
    assert _bits_of_floats(list(dlv.to_dict().values())) == got and list(dlv.to_dict()) == list(names)


def test_pack_on_a_real_forward_train_dict(real):
    from thinktwice_amd import logvars, losses as LS
    m, losses = real
    loss0, floats = LS.parse_losses(losses)
    loss1, dlv = m._parse_losses(losses, device_log=True)
    assert isinstance(dlv, logvars.DeviceLogVars) and dlv.names == tuple(floats) and len(dlv) == 24
    assert all(np.isfinite(v) for v in floats.values())
    assert _bits(dlv.packed) == _bits_of_floats(list(floats.values())), (dlv.packed.tolist(), floats)
    assert _bits(loss1.reshape(1)) == _bits(loss0.reshape(1))
    assert loss1.data_ptr() == dlv.packed.data_ptr() + 4 * 23
    # the default is what it was: floats
    assert all(isinstance(v, float) for v in floats.values())


def test_65_terms_raise():
    from thinktwice_amd import logvars
    with pytest.raises(ValueError, match="65"):
        logvars.pack(OrderedDict((f"t{i}_loss", _t(1.0)) for i in range(65)))
    with pytest.raises(ValueError, match="65"):
        logvars.pack(OrderedDict(a_loss=[_t(1.0)] * 64, b=_t(2.0)))


def test_terms_the_kernel_does_not_take_still_match():
    from thinktwice_amd import logvars, losses as LS
    rng = np.random.default_rng(2)
    many = torch.from_numpy(rng.normal(size=(2, 1)).astype(np.float32)).cuda()
    wide = torch.from_numpy(rng.normal(size=(3, 5)).astype(np.float32)).cuda()
    for dev in (OrderedDict(v_loss=many, w_loss=_t(0.25), x=[wide, _t(1.0)]),                  # more than one element
                OrderedDict(v_loss=_t(0.5).double(), w_loss=_t(0.25)),                          # another dtype
                OrderedDict(v_loss=torch.tensor(0.5), w_loss=torch.tensor(0.25))):              # host tensors
        _, floats = LS.parse_losses(dev)
        names, packed, loss = logvars.pack(dev)
        assert names == tuple(floats) and _bits(packed) == _bits_of_floats(list(floats.values()))
        assert _bits(loss.detach().float().reshape(1)) == _bits(packed[-1:])


# ------------------------------------------------------------------------------------------------- accumulate / flush
SENTINEL = -1234.5
WEIGHTS = [1, 2, 3, 4, 5, 6, 7, 8, 5]


def _accumulate_run(n, n_tail, seed):
    """9 good adds and two gated ones (NaN, Inf) into a window with sentinels around it; -> (window bits before the flush, out
    bits, window bits after, sentinels ok, expected flushed list)."""
    from thinktwice_amd._lib import check, cur_stream, lib
    rng = np.random.default_rng(seed)
    n_all = n + n_tail
    vals = (rng.choice([-1.0, 1.0], size=(9, n_all + 1)) * 10.0 ** rng.uniform(-30, 30, size=(9, n_all + 1))).astype(np.float32)
    packed = torch.from_numpy(vals[:, :n].copy()).cuda()
    tail = torch.from_numpy(vals[:, n:n + 2].copy()).cuda()              # 2 wide like grad_norm's [norm, factor]: [0] is read
    gates = torch.tensor([[1.0, 0.0], [float("nan"), 0.0], [float("inf"), 0.0], [-float("inf"), 0.0]], device="cuda")
    buf = torch.full((n_all + 3 + 4,), SENTINEL, dtype=torch.float64, device="cuda")
    obuf = torch.full((n_all + 3 + 4,), SENTINEL, dtype=torch.float64, device="cuda")
    window, out = buf[2:2 + n_all + 3], obuf[2:2 + n_all + 3]
    window.zero_()
    st = cur_stream(window.device)
    ref = R.HostWindow(n_all)

    def add(i, weight, gate):
        g = None if gate is None else gates[gate]
        check(lib().tt_logvars_accumulate(packed[i].data_ptr(), n, tail[i].data_ptr() if n_tail else None, n_tail, weight,
                                          None if g is None else g.data_ptr(), window.data_ptr(), st), "tt_logvars_accumulate")
        ref.add([float(x) for x in vals[i, :n_all]], weight, None if g is None else float(g[0]))

    for i, wgt in enumerate(WEIGHTS):
        add(i, wgt, 0 if i % 2 else None)                                # a finite gate or none: the add happens
        if i == 3:
            add(i, wgt, 1)                                               # NaN gate: skipped += 1 only
        if i == 6:
            add(i, wgt, 2)                                               # Inf gates
            add(i, wgt, 3)
    before = buf.cpu().clone()
    check(lib().tt_logvars_flush(window.data_ptr(), n_all + 3, out.data_ptr(), st), "tt_logvars_flush")
    torch.cuda.synchronize()
    return before, obuf.cpu(), buf.cpu(), ref.flush()


@pytest.mark.parametrize("n_tail", [0, 1])
@pytest.mark.parametrize("n", [1, 24, 64])
def test_accumulate_and_flush_equal_the_python_float_loop(n, n_tail):
    n_all = n + n_tail
    before, out, after, want = _accumulate_run(n, n_tail, seed=100 * n + n_tail)
    want_bits = [R.bits64(x) for x in want]
    bits = lambda t: t.view(torch.int64).tolist()                        # noqa: E731
    as_i64 = [b - (1 << 64) if b >= (1 << 63) else b for b in want_bits]
    assert want[n_all:] == [float(sum(WEIGHTS)), 9.0, 3.0]
    assert bits(before[2:-2]) == as_i64, (before[2:-2].tolist(), want)
    assert bits(out[2:-2]) == as_i64                                     # the flush hands over the same bits ...
    assert bits(after[2:-2]) == [0] * (n_all + 3)                        # ... and leaves +0.0 everywhere
    for t in (before, out, after):
        assert t[:2].tolist() == [SENTINEL] * 2 and t[-2:].tolist() == [SENTINEL] * 2
    again = _accumulate_run(n, n_tail, seed=100 * n + n_tail)
    assert bits(again[0]) == bits(before) and bits(again[1]) == bits(out)


def test_bad_arguments_are_refused():
    from thinktwice_amd import _lib
    L = _lib.lib()
    w = torch.zeros(8, dtype=torch.float64, device="cuda")
    p = torch.zeros(4, device="cuda")
    st = _lib.cur_stream(w.device)
    assert L.tt_logvars_accumulate(p.data_ptr(), 4, None, 1, 1, None, w.data_ptr(), st) != 0         # a tail count, no tail
    assert L.tt_logvars_accumulate(p.data_ptr(), 4, None, 0, 0, None, w.data_ptr(), st) != 0         # weight 0
    assert L.tt_logvars_accumulate(p.data_ptr(), 4, None, 0, 1 << 29, None, w.data_ptr(), st) != 0   # weight 2^29
    assert L.tt_logvars_flush(w.data_ptr(), 7, w.data_ptr() + 8, st) != 0                            # out overlaps window
    tab = _lib.structs()["tt_logvars_terms"]()
    tab.term[0] = tab.term[1] = p.data_ptr()
    tab.slot[0], tab.slot[1] = 0, 2
    assert L.tt_logvars_pack(ctypes.byref(tab), 2, 2, p.data_ptr(), st) != 0                         # slot 1 has no term
    assert L.tt_logvars_pack(ctypes.byref(tab), 65, 1, p.data_ptr(), st) != 0
    torch.cuda.synchronize()
    assert w.tolist() == [0.0] * 8 and p.tolist() == [0.0] * 4


# ------------------------------------------------------------------------------------------------------ the Python side
def test_log_window_names_and_results():
    from thinktwice_amd import logvars
    dev = torch.device("cuda", torch.cuda.current_device())
    win = logvars.LogWindow(dev)
    with pytest.raises(ValueError, match="nothing"):
        win.close()
    names = ("a_loss", "b", "loss")
    norm = torch.tensor([3.0, 1.0], device="cuda")
    rows = [[1.0, 2.0, 1.0], [0.5, -4.0, 0.5], [1e-3, 7.0, 1e-3]]
    ref = R.HostWindow(4)
    for row, wgt in zip(rows, (2, 1, 2)):
        win.add(logvars.DeviceLogVars(names, _t(row)), wgt, gate=norm, extra={"grad_norm": norm})
        ref.add([float(np.float32(x)) for x in row] + [3.0], wgt, 3.0)
    assert win.names == names + ("grad_norm",) and win.adds == 3
    with pytest.raises(ValueError, match="differ"):
        win.add(logvars.DeviceLogVars(("a_loss", "c", "loss"), _t(rows[0])), 1, gate=norm, extra={"grad_norm": norm})
    with pytest.raises(ValueError, match="differ"):
        win.add(logvars.DeviceLogVars(names, _t(rows[0])), 1)
    pending = win.close()
    assert win.adds == 0
    # the next window fills while the closed one is still unread
    win.add(logvars.DeviceLogVars(names, _t(rows[1])), 4, gate=torch.tensor([float("nan")], device="cuda"), extra={"grad_norm": norm})
    second = win.close()
    got, want = pending.result(), R.window_means(win.names, ref.flush())
    assert pending.ready() and list(got) == list(want)
    assert [R.bits64(v) for v in got.values()] == [R.bits64(v) for v in want.values()]
    assert got["num_samples"] == 5 and got["iterations"] == 3 and got["skipped"] == 0
    empty = second.result()                                              # no good iteration: NaN means, and it says so
    assert empty["iterations"] == 0 and empty["skipped"] == 1 and empty["num_samples"] == 0
    assert all(v != v for k, v in empty.items() if k in win.names)
    with pytest.raises(ValueError, match="65"):
        logvars.LogWindow(dev).add(logvars.DeviceLogVars(tuple(f"n{i}" for i in range(65)), torch.zeros(65, device="cuda")), 1)


def test_nothing_on_the_device_log_path_synchronises(real, monkeypatch):
    from thinktwice_amd import logvars
    m, losses = real
    norm = torch.tensor([2.0, 1.0], device="cuda")
    torch.cuda.synchronize()

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called on the device-log path: a host synchronisation")
        return f

    with monkeypatch.context() as mp:
        for name in ("item", "tolist", "cpu", "numpy", "__bool__"):
            mp.setattr(torch.Tensor, name, refuse("Tensor." + name))
        mp.setattr(torch.cuda, "synchronize", refuse("torch.cuda.synchronize"))
        mp.setattr(torch.cuda.Event, "synchronize", refuse("Event.synchronize"))
        mp.setattr(torch.cuda.Stream, "synchronize", refuse("Stream.synchronize"))
        loss, dlv = m._parse_losses(losses, device_log=True)
        win = logvars.LogWindow(m.device)
        win.add(dlv, B, gate=norm, extra={"grad_norm": norm})
        win.add(dlv, B, gate=norm, extra={"grad_norm": norm})
        pending = win.close()
        assert pending.ready() in (True, False)
    res = pending.result()                                               # the one call allowed to wait
    assert res["iterations"] == 2 and res["num_samples"] == 2 * B and res["grad_norm"] == 2.0
    assert [R.bits64(res[k]) for k in dlv.names] == [R.bits64(float(v)) for v in dlv.packed.tolist()]
