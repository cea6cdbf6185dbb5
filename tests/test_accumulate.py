"""Gradient accumulation on the GPU: Trainer.step(window=(j, k)) and EpochRunner(cumulative_iters=k), at the small
configuration of tests/test_train_step.py (final_dim 128 x 256, num_points 4096, B = 1 or 2, f32x3).  Two identically seeded
frozen-BN trainers are built once for the file; every test puts the one(s) it uses back to the initial checkpoint first.  The
comparisons are of bits unless a bound is stated."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu
HW = (128, 256)


def _batch(B, seed):
    from thinktwice_amd import model as tm, synth
    batch = tm.batch_to_device(synth.make_batch(B, img_hw=HW, num_points=4096, seed=seed))
    batch.update(synth.make_train_targets(B, img_hw=HW, seed=seed + 1))
    return batch


class _Rig:
    pass


@pytest.fixture(scope="module")
def rig():
    from thinktwice_amd import model as tm, params
    from thinktwice_amd.trainer import Trainer
    r = _Rig()
    m1, r.cfg = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    m2, _ = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    r.sd = params.init_params(r.cfg, seed=0)
    r.main, r.twin = Trainer(m1, r.sd, lr=1e-4), Trainer(m2, r.sd, lr=1e-4)
    r.A, r.B, r.C = _batch(1, 3), _batch(1, 13), _batch(1, 23)
    r.ck0 = r.main.checkpoint()
    return r


def _reset(*trainers, ck):
    for t in trainers:
        t.load_checkpoint(ck)
        assert not t.window_open and (t.iteration, t.opt.steps) == (0, 0)


@pytest.fixture(scope="module")
def grads(rig):
    """gA, gB, gC of Trainer.backward on the twin at the initial weights (A twice: the backward gives the same bits), kept
    unchanged for the tests that need them, and the twin's live ranges."""
    _reset(rig.twin, ck=rig.ck0)
    out = {}
    for name, batch in (("A", rig.A), ("A2", rig.A), ("B", rig.B), ("C", rig.C)):
        rig.twin.backward(batch)
        out[name] = rig.twin.grads.flat.clone()
    out["live"] = list(rig.twin.live_ranges)
    return out


def _live_mask(t, ranges):
    live = torch.zeros(t.flat_param.numel(), dtype=torch.bool, device=t.flat_param.device)
    for off, cnt in ranges:
        live[off:off + cnt] = True
    return live


def test_a_window_of_one_is_the_plain_step(rig):
    """window=(0, 1) against window=None, two steps each: 1.0 * g deposited by tt_grad_gather is g."""
    _reset(rig.main, rig.twin, ck=rig.ck0)
    for batch in (rig.A, rig.B):
        a = rig.main.step(batch, window=(0, 1))
        b = rig.twin.step(batch)
        assert a["updated"] is True and not rig.main.window_open
        assert torch.equal(a["grad_norm"], b["grad_norm"]) and torch.isfinite(a["grad_norm"]).all()
        assert torch.equal(rig.main.grads.flat, rig.twin.grads.flat)
    for x, y in ((rig.main.flat_param, rig.twin.flat_param), (rig.main.opt.m, rig.twin.opt.m), (rig.main.opt.v, rig.twin.opt.v)):
        assert torch.equal(x, y)
    assert rig.main.opt.steps == rig.twin.opt.steps == 2 and rig.main.iteration == rig.twin.iteration == 2
    assert rig.main.live_ranges == rig.twin.live_ranges


def test_backward_hands_over_the_tape_gradients_bit_for_bit(rig):
    """Trainer.backward over a buffer full of NaN: the flat gradient is, bit for bit, a zeroed buffer into which every
    `param_grads` entry is copied at its parameter's offset with torch; nothing outside `live_ranges` is written after the
    zeroing, and `live_ranges` are the merged runs of the reached parameters."""
    _reset(rig.main, ck=rig.ck0)
    t = rig.main
    t.grads.flat.fill_(float("nan"))
    t.backward(rig.A)
    got = t.grads.flat.clone()
    want, runs = torch.zeros_like(got), []
    for name, off in zip(t.names, t.grads.offsets):
        g = t.param_grads.get(name)
        if g is None:
            continue
        n = t.sd[name].numel()
        want[off:off + n].copy_(g.reshape(-1))
        if runs and runs[-1][1] == off:
            runs[-1][1] = off + n
        else:
            runs.append([off, off + n])
    assert set(t.param_grads) <= set(t.names) and 0 < len(t.param_grads) < len(t.names)
    assert not torch.isnan(got).any()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert t.live_ranges == [(a, b - a) for a, b in runs]
    dead = ~_live_mask(t, t.live_ranges)
    assert int(dead.sum()) > 0 and not got[dead].any()


def test_two_micro_steps_are_the_update_on_the_scaled_sum(rig, grads):
    """k = 2 on two different batches: after micro-step 0 the buffer is f32(0.5 * gA) and nothing else has happened; the close is
    clip + AdamW + re-preparation on f32(0.5 * gA) + f32(0.5 * gB), which the twin is handed directly."""
    assert torch.equal(grads["A"], grads["A2"])                           # the backward is bit-reproducible
    assert not torch.equal(grads["A"], grads["B"])
    _reset(rig.main, rig.twin, ck=rig.ck0)
    main, twin = rig.main, rig.twin
    p0 = main.flat_param.clone()
    first = main.step(rig.A, window=(0, 2))
    assert first["grad_norm"] is None and first["updated"] is False and main.window_open
    gA, gB = grads["A"].cpu().numpy(), grads["B"].cpu().numpy()
    half = np.float32(0.5)
    assert np.array_equal(main.grads.flat.cpu().numpy(), half * gA)
    assert torch.equal(main.flat_param, p0) and main.opt.issued == 0 and main.iteration == 1
    out = main.step(rig.B, window=(1, 2))
    assert out["updated"] is True and not main.window_open and main.iteration == 2 and main.opt.steps == 1
    want = (half * gA).astype(np.float32) + (half * gB).astype(np.float32)
    assert want.dtype == np.float32
    assert np.array_equal(main.grads.flat.cpu().numpy(), want)            # (AdamW does not write the gradient)
    twin.grads.flat.copy_(torch.from_numpy(want))
    assert main.live_ranges == grads["live"]                              # A and B reach the same parameters: the union is it
    norm = twin.opt.step(None, live_ranges=grads["live"])
    twin._prepare()
    assert torch.equal(out["grad_norm"], norm)
    for x, y in ((main.flat_param, twin.flat_param), (main.opt.m, twin.opt.m), (main.opt.v, twin.opt.v)):
        assert torch.equal(x, y)
    # dead ranges: zero gradient, untouched by AdamW (no weight decay either)
    dead = ~_live_mask(main, main.live_ranges)
    assert 0 < int(dead.sum()) < dead.numel() // 10
    assert not main.grads.flat[dead].any() and torch.equal(main.flat_param[dead], p0[dead])
    assert not torch.equal(main.flat_param[~dead], p0[~dead])
    # the re-prepared operands are the twin's: the next loss agrees
    assert float(main.model.train_step(rig.C, None)["loss"]) == float(twin.model.train_step(rig.C, None)["loss"])


def test_three_micro_steps_within_the_rounding_bound(rig, grads):
    """k = 3: |acc - (gA + gB + gC) / 3| <= 1.5 * 2^-24 * (|gA| + |gB| + |gC|) elementwise, right side in f64.  Derived: the
    scale is one rounding of 1/3, every product rounds once, every add rounds once -- a term passes through at most four
    roundings, (1 + 2^-24)^4 - 1 < 4.01 * 2^-24, on a third of its magnitude: 1.34 * 2^-24 * sum |g|."""
    _reset(rig.main, ck=rig.ck0)
    main = rig.main
    for j, batch in enumerate((rig.A, rig.B, rig.C)):
        out = main.step(batch, window=(j, 3))
        assert out["updated"] is (j == 2) and main.window_open is (j < 2)
    acc = main.grads.flat.double()
    gs = [grads[n].double() for n in "ABC"]
    err = (acc - (gs[0] + gs[1] + gs[2]) / 3.0).abs()
    bound = 1.5 * 2.0 ** -24 * (gs[0].abs() + gs[1].abs() + gs[2].abs())
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("k = 3: worst |error| / bound", worst, "elements over", int((err > bound).sum()))
    assert bool((err <= bound).all())
    assert float(err.max()) > 0.0 and main.opt.steps == 1 and main.iteration == 3


def test_a_skipped_window_leaves_no_trace(rig, grads):
    """Micro-step 0's deposit is made non-finite (one NaN written into the buffer, as
    test_non_finite_gradient_norm_skips_the_update_on_the_device poisons its gradient), micro-step 1 is clean: the close skips
    on the device, reconcile() takes both micro-iterations back, and the next window -- whose first deposit OVERWRITES -- is
    the one a trainer that never saw the bad window takes."""
    _reset(rig.main, rig.twin, ck=rig.ck0)
    main, twin = rig.main, rig.twin
    warm = main.step(rig.C, window=(0, 1), check_finite=False)            # one applied update first: m, v, steps are not zeros
    twin.step(rig.C, window=(0, 1), check_finite=False)
    assert warm["updated"] and main.reconcile() == 0
    start = main.iteration
    p, m, v = main.flat_param.clone(), main.opt.m.clone(), main.opt.v.clone()
    main.step(rig.A, window=(0, 2), check_finite=False)
    main.grads.flat[grads["live"][0][0] + 5] = float("nan")
    out = main.step(rig.B, window=(1, 2), check_finite=False)
    assert out["updated"] is True and main.iteration == start + 2         # the host ran ahead
    ns = out["grad_norm"].cpu()
    assert not torch.isfinite(ns[0]) and ns[1] != ns[1]
    assert torch.equal(main.flat_param, p) and torch.equal(main.opt.m, m) and torch.equal(main.opt.v, v)
    assert main.opt.steps == 1 and main.opt.skipped_iters() == 2
    assert main.reconcile() == 1 and main.iteration == start and main.reconcile() == 0
    assert not main.window_open
    for t in (main, twin):
        t.step(rig.A, window=(0, 2), check_finite=False)
        t.step(rig.B, window=(1, 2), check_finite=False)
    assert torch.isfinite(main.grads.flat).all() and torch.equal(main.grads.flat, twin.grads.flat)
    for x, y in ((main.flat_param, twin.flat_param), (main.opt.m, twin.opt.m), (main.opt.v, twin.opt.v)):
        assert torch.equal(x, y)
    assert main.opt.steps == twin.opt.steps == 2 and main.iteration == twin.iteration == start + 2
    # check_finite=True raises at the close and has taken the window back by then
    main.step(rig.A, window=(0, 2))
    main.grads.flat[grads["live"][0][0] + 5] = float("inf")
    with pytest.raises(FloatingPointError, match="non-finite"):
        main.step(rig.B, window=(1, 2))
    assert main.iteration == start + 2 and not main.window_open and main.opt.steps == 2 and main.reconcile() == 0
    assert torch.equal(main.flat_param, twin.flat_param)


def test_order_errors_come_before_any_launch(rig):
    from thinktwice_amd._lib import TTError
    _reset(rig.main, ck=rig.ck0)
    main = rig.main
    p0 = main.flat_param.clone()
    with pytest.raises(ValueError, match="no window open"):
        main.step(rig.A, window=(1, 2))
    with pytest.raises(ValueError):
        main.step(rig.A, window=(2, 2))
    assert not main.window_open and main.iteration == 0
    main.step(rig.A, window=(0, 2))
    g = main.grads.flat.clone()
    with pytest.raises(ValueError, match="does not continue"):
        main.step(rig.B, window=(1, 3))
    with pytest.raises(ValueError, match="does not continue"):
        main.step(rig.B, window=(0, 2))                                   # a gap in j: micro-step 1 is due
    with pytest.raises(ValueError, match="window=None"):
        main.step(rig.B)
    for call in (main.checkpoint, main.state_dict, main.optimizer_state_dict):
        with pytest.raises(TTError, match="window open"):
            call()
    assert main.window_open and main.iteration == 1 and main.opt.issued == 0
    assert torch.equal(main.flat_param, p0) and torch.equal(main.grads.flat, g)
    out = main.step(rig.B, window=(1, 2))                                 # the window is still the one that was open
    assert out["updated"] and main.checkpoint()["meta"]["iter"] == 2
    # a plain step after window closes, and a window after plain steps: the trainer squares its bookkeeping where the form changes
    plain = main.step(rig.C, check_finite=False)
    assert "updated" not in plain and main.iteration == 3
    main.step(rig.A, window=(0, 1), check_finite=False)
    assert main.reconcile() == 0 and main.iteration == 4 and main.opt.steps == 3


def test_train_mode_counters_move_on_every_micro_step():
    """frozen_bn=False, one closed window of two: the BatchNorm call counters have two calls' worth, the running statistics
    moved again on micro-step 1, the Adam step count is 1."""
    from thinktwice_amd import model as tm, params
    from thinktwice_amd.trainer import Trainer
    m, cfg = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    sd0 = params.init_params(cfg, seed=0)
    tr = Trainer(m, sd0, lr=1e-4, frozen_bn=False)
    b0, b1 = _batch(2, 3), _batch(2, 13)
    k_stat = "img_encoder.img_backbone.bn1.running_mean"
    tr.step(b0, window=(0, 2))
    after0 = tr.buffers[k_stat].clone()
    assert float((after0.cpu() - sd0[k_stat]).abs().max()) > 0
    out = tr.step(b1, window=(1, 2))
    assert out["updated"] and torch.isfinite(out["grad_norm"]).all()
    assert float((tr.buffers[k_stat] - after0).abs().max()) > 0
    state = tr.state_dict()
    k_cam = "img_encoder.img_backbone.bn1.num_batches_tracked"
    k_lid = next(k for k in sd0 if k.startswith("lidar_encoder.") and k.endswith("num_batches_tracked"))
    assert int(state[k_cam]) == int(sd0[k_cam]) + 4 and int(state[k_lid]) == int(sd0[k_lid]) + 2
    osd = tr.optimizer_state_dict()
    assert osd["state"] and all(float(s["step"]) == 1.0 for s in osd["state"].values())
    assert tr.iteration == 2 and tr._bn_steps == 2 and tr.opt.steps == 1


def test_a_skipped_plain_step_and_a_skipped_window_are_counted_by_their_own_rules():
    """frozen_bn=False, a batch whose gradient norm is not finite (a NaN in the Beta target action_mu, as test_runner.Poisoned
    makes one), check_finite=False: the device skips the update, reconcile() finds one skip and takes the iteration back.
    `_bn_steps` goes back with a plain step and stays with a window (its forward ran and moved the running statistics).
    check_finite=True on the plain step raises before the counters move, and reconcile() has nothing left to find."""
    from thinktwice_amd import model as tm, params
    from thinktwice_amd.trainer import Trainer
    m, cfg = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    tr = Trainer(m, params.init_params(cfg, seed=0), lr=1e-4, frozen_bn=False)
    ck0, p0 = tr.checkpoint(), tr.flat_param.clone()
    bad = dict(_batch(2, 3))
    bad["action_mu"] = bad["action_mu"].clone()
    bad["action_mu"].view(-1)[0] = float("nan")
    for window, bn_steps in ((None, 0), ((0, 1), 1)):
        tr.load_checkpoint(ck0)
        out = tr.step(bad, check_finite=False, window=window)
        assert not torch.isfinite(out["grad_norm"][0]) and ("updated" in out) is (window is not None)
        assert tr.reconcile() == 1
        assert (tr.iteration, tr.opt.steps, tr._bn_steps) == (0, 0, bn_steps), window
        assert torch.equal(tr.flat_param, p0)
    tr.load_checkpoint(ck0)
    with pytest.raises(FloatingPointError, match="non-finite"):
        tr.step(bad)
    assert tr.iteration == 0 and tr.reconcile() == 0 and tr.iteration == 0 and tr._bn_steps == 0
    assert tr.opt.steps == 0 and torch.equal(tr.flat_param, p0)


def test_the_autograd_route_accumulates_the_same_bits(rig):
    """A ten-line cumulative hook on a trainable=True model -- (loss / 2).backward() twice, no zero_grad between -- leaves in
    every parameter's .grad the bits of the Trainer's flat buffer after its two deposits: scale, then add, both ways."""
    from thinktwice_amd import model as tm
    _reset(rig.main, ck=rig.ck0)
    main = rig.main
    main.step(rig.A, window=(0, 2))
    main.step(rig.B, window=(1, 2))
    m, _ = tm.build_thinktwice(final_dim=HW, dtype="f32x3", trainable=True)
    m.load_state_dict(rig.sd)
    m.eval()                                                              # the rig's trainers are frozen-BN
    m.zero_grad()
    k = 2
    for i, batch in enumerate((rig.A, rig.B)):                            # GradientCumulativeOptimizerHook.after_train_iter
        loss = m.train_step(batch, None)["loss"]
        (loss / k).backward()
        if (i + 1) % k == 0:
            pass                                                          # (clip + optimizer.step() + zero_grad() would go here)
    named = dict(m.named_parameters())
    assert list(named) == main.names
    none = 0
    for name in main.names:
        got, want = named[name].grad, main.sd[name].grad
        if got is None:
            none += 1
            assert not want.any(), name
        else:
            assert torch.equal(got, want), name
    assert 0 < none < len(main.names) // 5


def _rank_window(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from thinktwice_amd import model as tm, params, synth
        from thinktwice_amd.trainer import Trainer
        m, cfg = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
        tr = Trainer(m, params.init_params(cfg, seed=0), lr=1e-4)
        calls, real = [], dist.all_reduce

        def counting(t, *a, **kw):                                         # the collectives over the whole flat gradient
            if t.numel() == tr.grads.numel:
                calls.append(1)
            return real(t, *a, **kw)

        dist.all_reduce = counting
        p0 = tr.flat_param[::997].cpu()
        for j in range(2):                                                 # every rank and micro-step its own sample
            batch = synth.make_batch(1, img_hw=HW, num_points=4096, seed=100 + 10 * j + rank)
            batch.update(synth.make_train_targets(1, img_hw=HW, seed=200 + 10 * j + rank))
            out = tr.step(batch, window=(j, 2))
            assert len(calls) == j
        torch.cuda.synchronize()
        p1 = tr.flat_param[::997].cpu()
        q.put((rank, len(calls), out["grad_norm"].cpu().numpy(), p1.numpy(), float(tr.flat_param.double().sum()),
               bool((p1 != p0).any()), tr.grads.flat[::997].cpu().numpy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_reduce_once_per_window_gloo():
    """world_size 2 on this box's one GPU (gloo, the scaffolding of test_two_rank_training_step_gloo): one k = 2 window per rank on
    rank-specific batches reaches the collective once, at the close, and leaves bit-identical parameters on both ranks."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_rank_window, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=600) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, n0, norm0, p0, sum0, moved0, g0), (_, n1, norm1, p1, sum1, moved1, g1) = got
    assert n0 == n1 == 1
    assert np.array_equal(norm0, norm1) and np.isfinite(norm0).all()
    assert np.array_equal(g0, g1) and np.array_equal(p0, p1) and sum0 == sum1 and moved0 and moved1


# ------------------------------------------------------------------------------------------------- the runner, end to end
def _runner_objects(tree):
    import dataset_cases as D
    from thinktwice_amd import calib, dataset, model as tm, ops, params
    from thinktwice_amd.loader import DeviceBatchLoader
    from thinktwice_amd.trainer import Trainer
    conf = dict(calib.IDA_AUG_CONF, final_dim=HW, resize_lim=(0.56 * 128 / 448, 0.6255 * 128 / 448))       # test_runner.py's
    ops.DROPOUT_SEED[:] = [0x5EED, 0]
    m, cfg = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    trainer = Trainer(m, params.init_params(cfg, seed=0), lr=1e-4, frozen_bn=False)
    index = dataset.DatasetIndex(tree["metadata"], ["town06_00"], D.CFG, root=tree["root"])
    loader = DeviceBatchLoader(index, D.CFG, conf, batch_size=2, seed=3, prefetch=2, threads=8, train=True)
    assert len(index) == 5 and len(loader) == 3                            # five samples, padded to three batches of two
    return trainer, loader


def _final(trainer):
    return {"state": trainer.state_dict(), "optimizer": trainer.optimizer_state_dict()}


def test_the_runner_accumulates_per_epoch_and_resumes_bit_identically(tmp_path):
    """n = 3 iterations per epoch, cumulative_iters = 2, two epochs: windows (0,2) (1,2) (0,1) per epoch, so four updates over
    six iterations; its checkpoint after one epoch, fresh objects, resume('auto'), one more epoch end where the straight run ends."""
    import json
    import shutil
    import dataset_cases as D
    from test_runner import _same
    from thinktwice_amd import ops
    from thinktwice_amd.runner import EpochRunner
    saved = list(ops.DROPOUT_SEED)
    os.makedirs(str(tmp_path / "tree"))
    tree = D.write_tree(tmp_path / "tree")
    try:
        trainer, loader = _runner_objects(tree)
        work = str(tmp_path / "whole")
        EpochRunner(trainer, loader, work_dir=work, max_epochs=2, log_interval=1, verbose=False, cumulative_iters=2).run()
        loader.close()
        assert trainer.opt.steps == 4 and trainer.iteration == 6 and not trainer.window_open
        with open(os.path.join(work, "log.json")) as f:
            lines = [json.loads(x) for x in f]
        assert [(x["epoch"], x["iter"], x["iterations"]) for x in lines] == [(1, 2, 2), (1, 3, 1), (2, 2, 2), (2, 3, 1)]
        assert sum(x["iterations"] for x in lines) == 6 and all(x["skipped"] == 0 and np.isfinite(x["loss"]) for x in lines)
        ckpt = torch.load(os.path.join(work, "latest.pth"), weights_only=False)
        assert ckpt["meta"]["iter"] == 6 and ckpt["meta"]["runner"]["cumulative_iters"] == 2
        whole = _final(trainer)
        del trainer

        # the interrupted run: the straight run's checkpoint after epoch [0] is what a run stopped there leaves behind
        work = str(tmp_path / "parts")
        os.makedirs(work)
        shutil.copyfile(os.path.join(str(tmp_path / "whole"), "epoch_1.pth"), os.path.join(work, "latest.pth"))
        trainer, loader = _runner_objects(tree)
        ops.DROPOUT_SEED[:] = [1, 99]                                     # fresh objects need not be in step: the state decides
        again = EpochRunner(trainer, loader, work_dir=work, max_epochs=2, log_interval=1, verbose=False, cumulative_iters=2)
        assert again.resume("auto") == 1 and trainer.iteration == 3 and trainer.opt.steps == 2
        again.run()
        loader.close()
        assert trainer.opt.steps == 4 and trainer.iteration == 6
        parts = _final(trainer)
        _same(whole["state"], parts["state"], "state_dict")               # parameters, running statistics, num_batches_tracked
        _same(whole["optimizer"], parts["optimizer"], "optimizer")        # moments, step counts, rates
    finally:
        ops.DROPOUT_SEED[:] = saved

