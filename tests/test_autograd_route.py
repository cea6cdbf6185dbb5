"""The torch-autograd route of the training step (thinktwice_amd/autograd_route.py): a `trainable=True` EncoderDecoder is the
module the reference's training lines expect -- real nn.Parameters under the reference's names, `loss.backward()` through the HIP
backward kernels, torch.optim.AdamW / clip_grad_norm_ / DistributedDataParallel on top, a live `state_dict()`.

mmcv is not a dependency: the loop below restates what OptimizerHook.after_train_iter amounts to
(zero_grad, loss.backward(), clip_grad_norm_(params, 100), step)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HW = (128, 256)
GOLD = os.path.join(os.path.dirname(__file__), "golden")
BOUND = 1e-4          # run-to-run bound of two backward sweeps (three f32-atomic scatters; tests/test_train_step.py)


def _batch(B, seed=3):
    from thinktwice_amd import model as tm, synth
    batch = tm.batch_to_device(synth.make_batch(B, img_hw=HW, num_points=4096, seed=seed))
    batch.update(synth.make_train_targets(B, img_hw=HW, seed=seed + 1))
    return batch


def _flat_grads(model):
    """Concatenated `.grad` of model.parameters() (zeros where it is None) and the names whose `.grad` is None."""
    parts, none = [], []
    for n, p in model.named_parameters():
        if p.grad is None:
            none.append(n)
            parts.append(torch.zeros(p.numel(), dtype=torch.float32, device=p.device))
        else:
            parts.append(p.grad.detach().reshape(-1))
    return torch.cat(parts), none


class _Rig:
    pass


@pytest.fixture(scope="module")
def rig():
    """One trainable model and one non-trainable twin under a Trainer (same seed, frozen BN), built once for the file."""
    from thinktwice_amd import model as tm, params
    from thinktwice_amd.trainer import Trainer
    r = _Rig()
    r.model, r.cfg = tm.build_thinktwice(final_dim=HW, dtype="f32x3", trainable=True)
    r.sd = params.init_params(r.cfg, seed=0)
    r.model.load_state_dict(r.sd)
    r.twin, _ = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    r.trainer = Trainer(r.twin, r.sd)
    r.batch = _batch(2)
    return r


# ------------------------------------------------------------------------------------------------------- module surface
def test_module_surface_parameters_state_dict_and_reload(rig):
    from thinktwice_amd import params
    m, sd = rig.model, rig.sd
    names = [n for n, _ in m.named_parameters()]
    assert names == rig.trainer.names and len(names) == 968
    assert list(m.state_dict()) == list(sd)
    assert all(p.is_cuda and p.dtype == torch.float32 and p.requires_grad for p in m.parameters())
    # the masters are views of one flat buffer, laid out like Trainer.flat_param
    ps = list(m.parameters())
    base = ps[0].data_ptr()
    off = 0
    for p in ps:
        assert p.data_ptr() == base + 4 * off
        off += p.numel()
    assert off == rig.trainer.flat_param.numel()
    # the default is unchanged: no parameters, no graph, the loaded dict as state_dict
    assert list(rig.twin.parameters()) == []
    assert rig.twin.train_step(rig.batch, None)["loss"].grad_fn is None
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-7)
    assert len(opt.param_groups[0]["params"]) == 968
    # load_state_dict on a trainable model: into the existing masters
    sd2 = params.init_params(rig.cfg, seed=1)
    ids = [id(p) for p in m.parameters()]
    m.load_state_dict(sd2)
    assert ids == [id(p) for p in m.parameters()]
    live = m.state_dict()
    for k in (names[0], names[100], names[-1], "img_encoder.img_backbone.bn1.running_var"):
        assert torch.equal(live[k].cpu(), sd2[k].float()), k
    assert opt.param_groups[0]["params"][5] is ps[5]
    m.load_state_dict(sd)
    assert torch.equal(m.state_dict()[names[100]].cpu(), sd[names[100]])


def test_guards(rig):
    from thinktwice_amd import _lib, model as tm
    from thinktwice_amd.trainer import Trainer
    for bad in ("f32x3h", torch.bfloat16, torch.float16):
        with pytest.raises(_lib.TTError):
            tm.build_thinktwice(final_dim=HW, dtype=bad, trainable=True)
    with pytest.raises(_lib.TTError):
        Trainer(rig.model, rig.sd)
    with pytest.raises(_lib.TTError):
        rig.model.to(torch.float16)
    with pytest.raises(_lib.TTError):
        rig.model.cpu()
    m = rig.model
    m.eval()
    with torch.no_grad():
        out = m.train_step(rig.batch, None)
    assert out["loss"].grad_fn is None and not out["loss"].requires_grad
    m.zero_grad()
    out = m.train_step(rig.batch, None)
    assert out["loss"].grad_fn is not None
    terms = m.forward_train(rig.batch)
    assert all(v.grad_fn is None for v in terms.values() if torch.is_tensor(v))      # only the parsed total carries the graph
    del terms                                                                        # (its tape goes with it)
    out["loss"].backward()
    with pytest.raises(RuntimeError, match="second time"):
        out["loss"].backward()
    m.zero_grad()


# ------------------------------------------------------------------------------- gradients against the reference (F13)
@pytest.mark.parametrize("mode,tol", [("f32", 2.5e-3), ("f32x3", 1e-2)], ids=["f13-f32", "f13-bf16x3"])
def test_loss_backward_matches_reference_gradients_golden_f13(mode, tol, monkeypatch):
    """`model.train_step(batch, None)["loss"].backward()` against the reference's own loss.backward() (golden F13, B = 2): the
    assertions and bounds of tests/test_train_step.py::test_training_backward_matches_reference_gradients_golden_f13, read
    from `p.grad` of named_parameters()."""
    from thinktwice_amd import autodiff, model as tm, params, synth
    pack = np.load(os.path.join(GOLD, "f13_train_gradients_b2.npz"))
    B, H, W, npts, seed = (int(v) for v in pack["meta"])
    m, cfg = tm.build_thinktwice(final_dim=(H, W), dtype=torch.float32 if mode == "f32" else "f32x3", trainable=True)
    m.load_state_dict(params.init_params(cfg, seed=seed))
    batch = synth.make_batch(B, img_hw=(H, W), num_points=npts)
    batch.update(synth.make_train_targets(B, img_hw=(H, W)))
    reached = []
    sweep = autodiff.Tape.backward

    def spy(self):
        sweep(self)
        reached.append(set(self.param_grads))

    monkeypatch.setattr(autodiff.Tape, "backward", spy)
    out = m.train_step(batch, None)
    out["loss"].backward()
    torch.cuda.synchronize()
    want_total = float(pack["total_loss"][0])
    assert abs(float(out["loss"].detach()) - want_total) < (1e-3 if mode == "f32" else 2e-3) * abs(want_total)
    grads = {n: p.grad for n, p in m.named_parameters()}
    live = [str(n) for n in pack["names"]]
    missing = [n for n in live if grads[n] is None]
    assert not missing, (len(missing), missing[:10])
    dead = sorted(str(k) for k in pack["dead"])
    got_dead = sorted(k for k, g in grads.items() if g is None or float(g.abs().max()) == 0.0)
    assert got_dead == dead, (sorted(set(got_dead) ^ set(dead))[:10])
    # a parameter the tape did not reach has no gradient at all -- None, not zeros (torch's AdamW then skips it)
    assert len(reached) == 1
    assert sorted(k for k, g in grads.items() if g is None) == sorted(set(grads) - reached[0])
    norm_err, samp_err = {}, {}
    for name, norm, idx, smp in zip(live, pack["norms"], pack["idx"], pack["samples"]):
        g = grads[name].detach().cpu()
        norm = float(norm)
        norm_err[name] = abs(float(g.norm()) - norm) / max(norm, 1e-12)
        got = g.reshape(-1)[torch.from_numpy(idx)].numpy()
        samp_err[name] = float(np.abs(got - smp).max()) / max(norm, 1e-12)
    wn = sorted(norm_err.items(), key=lambda kv: -kv[1])[:5]
    ws = sorted(samp_err.items(), key=lambda kv: -kv[1])[:5]
    ne = np.array(list(norm_err.values()))
    print(mode, "params", len(live), "worst norm rel", wn[0], "worst sample/norm", ws[0],
          "median norm rel", float(np.median(ne)), "share of parameters within 1e-3:", float((ne < 1e-3).mean()))
    assert wn[0][1] < tol, wn
    assert ws[0][1] < tol, ws
    assert float((ne < 1e-3).mean()) >= (0.995 if mode == "f32" else 0.90), float((ne < 1e-3).mean())
    assert float(np.median(ne)) < (5e-5 if mode == "f32" else 5e-4)


# ----------------------------------------------------------------------------------- against the Trainer on a twin model
def test_loss_and_gradients_equal_the_trainer_on_a_twin_model(rig):
    """Same seed, same batch, frozen BN.  The yardstick for the loss is the existing code itself: two Trainer.backward calls on
    one batch (expected: no difference at all); for the gradients the run-to-run bound of two backward sweeps."""
    m, tr, batch = rig.model, rig.trainer, rig.batch
    m.eval()
    l1 = float(tr.backward(batch)["loss"])
    l2 = float(tr.backward(batch)["loss"])
    g = tr.grads.flat.clone()
    gn = float(g.norm())
    m.zero_grad()
    out = m.train_step(batch, None)
    out["loss"].backward()
    got, none = _flat_grads(m)
    print("trainer losses", l1, l2, "route loss", float(out["loss"].detach()), "grad diff / norm", float((got - g).norm()) / gn)
    assert abs(float(out["loss"].detach()) - l1) <= abs(l1 - l2)
    assert float((got - g).norm()) <= BOUND * gn
    assert sorted(none) == sorted(k for k in tr.names if k not in tr.param_grads) and len(none) == 90
    # grad_output is a device scalar, applied on the device: (loss * 0.5).backward() gives half
    m.zero_grad()
    (m.train_step(batch, None)["loss"] * 0.5).backward()
    half, _ = _flat_grads(m)
    print("half: diff / norm", float((half - 0.5 * g).norm()) / (0.5 * gn))
    assert float((half - 0.5 * g).norm()) <= BOUND * 0.5 * gn
    # gradient accumulation is AccumulateGrad's: two backward() calls of two train_steps without zero_grad give the sum
    m.zero_grad()
    m.train_step(batch, None)["loss"].backward()
    m.train_step(batch, None)["loss"].backward()
    both, none2 = _flat_grads(m)
    print("sum: diff / norm", float((both - 2.0 * g).norm()) / (2.0 * gn))
    assert float((both - 2.0 * g).norm()) <= BOUND * 2.0 * gn
    assert sorted(none2) == sorted(none)
    m.zero_grad()


def test_train_mode_running_statistics_and_call_counters_equal_the_trainer(rig):
    """model.train(): the running statistics after one train_step equal those of Trainer(frozen_bn=False).backward on a fresh
    twin (they depend on the forward only; same dropout masks on both sides); allowed difference: what two fresh twins show
    between themselves.  num_batches_tracked follows Trainer._num_batches_tracked."""
    from thinktwice_amd import model as tm, ops
    from thinktwice_amd.trainer import Trainer
    sd, batch = rig.sd, rig.batch
    mid = rig.cfg["img_encoder"]["depth_net_conf"]["mid_channels"]
    mask = (torch.rand(2 * 2 * 4, HW[0] // 16, HW[1] // 16, mid, generator=torch.Generator().manual_seed(5)) > 0.5).to(torch.uint8)

    def run(step):
        ops.DROPOUT_MASKS = iter([mask])
        try:
            return step()
        finally:
            ops.DROPOUT_MASKS = None

    trs = []
    for _ in range(2):
        twin, _c = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
        trs.append(Trainer(twin, sd, frozen_bn=False))
        run(lambda: trs[-1].backward(batch))
    m, _c = tm.build_thinktwice(final_dim=HW, dtype="f32x3", trainable=True)
    m.load_state_dict(sd)
    m.train()
    out = run(lambda: m.train_step(batch, None))
    torch.cuda.synchronize()
    live = m.state_dict()
    worst, moved = 0.0, 0
    for k, b in trs[0].buffers.items():
        allowed = float((b - trs[1].buffers[k]).abs().max())
        diff = float((live[k] - b).abs().max())
        worst = max(worst, diff - allowed)
        moved += int(float((b.cpu() - sd[k]).abs().max()) > 0)
        assert diff <= allowed, (k, diff, allowed)
    print("running statistics:", len(trs[0].buffers), "buffers,", moved, "moved, worst excess over twin-vs-twin", worst)
    assert moved > 100
    # one applied iteration on the Trainer side: its state_dict advances the counters by the same rule
    run(lambda: trs[0].step(batch))
    want = trs[0].state_dict()
    k_cam = "img_encoder.img_backbone.bn1.num_batches_tracked"
    assert int(live[k_cam]) == int(sd[k_cam]) + 2
    for k, v in want.items():
        if k.endswith("num_batches_tracked"):
            assert int(live[k]) == int(v), k
    out["loss"].backward()          # the train-mode tape sweeps too
    assert sum(p.grad is not None for p in m.parameters()) >= 878


# ------------------------------------------------------------------------------------------------- the reference's loop
def test_the_reference_training_loop_runs_on_the_model(rig, monkeypatch):
    """OptimizerHook's lines with torch's own AdamW and clip: the loss falls, dead parameters are left exactly alone and carry
    no optimizer state, and afterwards the model runs on the UPDATED weights -- its forward equals, bit for bit, the forward of
    a fresh non-trainable model loaded with its state_dict() (operand refresh + live state_dict)."""
    from thinktwice_amd import masters, model as tm
    m, sd, batch = rig.model, rig.sd, rig.batch
    pack = np.load(os.path.join(GOLD, "f13_train_gradients_b2.npz"))
    dead = [str(k) for k in pack["dead"]]
    m.load_state_dict(sd)
    m.eval()                                                   # frozen-BN fine-tuning, as Trainer's default
    m.zero_grad()
    calls = []
    prepare = masters.prepare_on_device
    monkeypatch.setattr(masters, "prepare_on_device", lambda *a, **k: (calls.append(1), prepare(*a, **k))[1])
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-7)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = m.train_step(batch, opt)
        out["loss"].backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 100)
        opt.step()
        losses.append(float(out["loss"].detach()))
    print("losses over 3 iterations of the reference's loop:", losses, "preparations:", len(calls))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert len(calls) == 2                                     # one per parameter write that a forward followed
    named = dict(m.named_parameters())
    for k in dead:
        assert torch.equal(named[k].detach().cpu(), sd[k]), k
    state = opt.state_dict()["state"]
    index = {n: i for i, n in enumerate(named)}
    assert not any(index[k] in state for k in dead)
    assert len(state) == len(pack["names"]) == 878
    assert any(not torch.equal(named[str(k)].detach().cpu(), sd[str(k)]) for k in pack["names"][:20])
    # the forward after the loop runs on the new values (one re-preparation), a second one on the same values (none)
    pred = m.forward_inference(batch)
    assert len(calls) == 3
    again = m.forward_inference(batch)
    with torch.no_grad():
        m.train_step(batch, None)
    assert len(calls) == 3
    fresh, _c = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    fresh.load_state_dict(m.state_dict())                      # the live tensors, on the device
    ref = fresh.forward_inference(batch)
    compared = 0
    for k, v in pred.items():
        items = v if isinstance(v, (list, tuple)) else [v]
        others = ref[k] if isinstance(v, (list, tuple)) else [ref[k]]
        for a, b in zip(items, others):
            if torch.is_tensor(a):
                assert torch.equal(a, b), k
                compared += 1
    assert compared >= 10 and torch.equal(pred["pred_wp"], again["pred_wp"])
    m.load_state_dict(sd)
    m.zero_grad()


# ------------------------------------------------------------------------------------------------------------------ DDP
def _ddp_child(port, q):
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from thinktwice_amd import model as tm, params
        m, cfg = tm.build_thinktwice(final_dim=HW, dtype="f32x3", trainable=True)
        m.load_state_dict(params.init_params(cfg, seed=0))
        batch = _batch(2)
        m.train_step(batch, None)["loss"].backward()
        g0, none0 = _flat_grads(m)
        m.zero_grad()
        before = m._masters.preparations
        ddp = DistributedDataParallel(m, device_ids=[0], broadcast_buffers=False, find_unused_parameters=True)
        out = ddp(**batch)
        prepared = m._masters.preparations - before       # DDP's constructor broadcast wrote the parameters in place: once
        out["loss"].backward()
        g1, none1 = _flat_grads(m)
        torch.cuda.synchronize()
        q.put(dict(prepared=prepared, rel=float((g1 - g0).norm()) / float(g0.norm()), none0=len(none0),
                   same_none=sorted(none0) == sorted(none1), loss=float(out["loss"].detach())))
    finally:
        dist.destroy_process_group()


def test_distributed_data_parallel_wraps_the_model_and_backward_completes():
    """torch's DistributedDataParallel (what MMDistributedDataParallel derives from) with the reference's arguments, one rank
    over RCCL, in a child process with one time limit and no retry."""
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_ddp_child, args=(29500 + (os.getpid() % 2000), q))
    p.start()
    got, waited = None, 0
    while got is None and waited < 420:                    # one time limit; a child that has died ends the wait at once
        try:
            got = q.get(timeout=5)
        except queue.Empty:
            waited += 5
            if not p.is_alive():
                break
    p.join(timeout=60)
    if p.is_alive():
        p.kill()
        p.join()
    assert got is not None and p.exitcode == 0, (got, p.exitcode)
    print("DDP child:", got)
    assert got["prepared"] == 1
    assert got["rel"] <= BOUND
    assert got["none0"] == 90 and got["same_none"]
    assert np.isfinite(got["loss"])
