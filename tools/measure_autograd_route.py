"""Numbers behind profiles/autograd_route.txt (one MI355X, the thinktwice.py size, f32x3):

  loop    a per-parameter `copy_` loop written here (`tr.sd[k].grad.copy_(g.reshape(...))`, one torch launch per gradient
          tensor: how Trainer.backward filled its flat buffer before it took the gather) on the real gradient tensors of one
          backward -- runs on any commit that has trainer.Trainer
  gather  tt_grad_gather on the same tensors' segment table: upload + one launch, and the launch alone; achieved bytes/s
  iter    one iteration of the torch-autograd route (trainable model, torch AdamW(foreach=True) + clip_grad_norm_) next to
          Trainer.step on the same batch, alternating, model.train() semantics on both sides

    python tools/measure_autograd_route.py loop gather iter --batch 8

Times are device events around repeated work after a warm-up (loop / gather) and a host clock around synchronised iterations
(iter); medians over the repeats, with the spread."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from thinktwice_amd import build, model as tm, params, synth  # noqa: E402
from thinktwice_amd.trainer import Trainer  # noqa: E402


def _events(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def _batch(B):
    batch = tm.batch_to_device(synth.make_batch(B, seed=1234))
    batch.update(synth.make_train_targets(B))
    return batch


def loop_and_gather(args, what):
    m, cfg = tm.build_thinktwice(dtype="f32x3")
    tr = Trainer(m, params.init_params(cfg, seed=0), frozen_bn=False)
    batch = _batch(args.batch)
    tr.backward(batch)
    grads = tr.param_grads
    n = sum(g.numel() for g in grads.values())
    print(f"gradient tensors of one backward at B = {args.batch}: {len(grads)} tensors, {n} floats, {4 * n / 1e6:.1f} MB")
    if "loop" in what:
        def loop():
            for k, g in grads.items():
                tr.sd[k].grad.copy_(g.reshape(tr.sd[k].shape))
        med, lo, hi = _events(loop, args.repeats)
        print(f"this tool's own copy_ loop ({len(grads)} launches): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) over {args.repeats} repeats; "
              f"{8 * n / med / 1e6:.1f} GB/s of read + write")
    if "gather" in what:
        from thinktwice_amd import ops
        flat = torch.empty_like(tr.grads.flat)
        offs, off = {}, 0
        for k in tr.names:
            offs[k] = off
            off += tr.sd[k].numel()
        srcs = [g.reshape(-1) for g in grads.values()]
        dst = [offs[k] for k in grads]
        table = ops.GradSegTable(flat.device)
        scale = torch.tensor([0.5], device=flat.device)
        med, lo, hi = _events(lambda: ops.grad_gather(table.upload(srcs, dst, flat.numel()), flat, scale), args.repeats)
        print(f"tt_grad_gather, table upload + one launch: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
        for name, kw in (("=, scaled", dict(scale=scale)), ("=, unscaled", dict()), ("+=, scaled", dict(scale=scale, accumulate=True))):
            med, lo, hi = _events(lambda: ops.grad_gather(table, flat, **kw), args.repeats)
            nbytes = (12 if kw.get("accumulate") else 8) * n
            print(f"tt_grad_gather alone ({name}): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}); "
                  f"{nbytes / med / 1e6:.1f} GB/s of read + write")
        ops.grad_gather(table, flat)
        want = torch.cat([tr.sd[k].grad.reshape(-1) if k in grads else torch.zeros(tr.sd[k].numel(), device=flat.device)
                          for k in tr.names])
        live = torch.cat([torch.full((tr.sd[k].numel(),), k in grads, dtype=torch.bool, device=flat.device) for k in tr.names])
        print("gathered buffer bit-equal to the copy_ loop's on the covered elements:",
              bool(torch.equal(flat[live].view(torch.int32), want[live].view(torch.int32))))


def iteration(args):
    batch = _batch(args.batch)
    m, cfg = tm.build_thinktwice(dtype="f32x3", trainable=True)
    sd = params.init_params(cfg, seed=0)
    m.load_state_dict(sd)
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-7, foreach=True)
    twin, _ = tm.build_thinktwice(dtype="f32x3")
    tr = Trainer(twin, sd, frozen_bn=False)

    def route():
        opt.zero_grad()
        out = m.train_step(batch, opt)
        out["loss"].backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 100, foreach=True)
        opt.step()

    times = {"route": [], "trainer": []}
    for i in range(args.warmup + args.steps):
        for name, fn in (("route", route), ("trainer", lambda: tr.step(batch))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    for name, ts in times.items():
        print(f"{name}: one iteration at B = {args.batch}: median {statistics.median(ts):.1f} ms (min {min(ts):.1f}, max {max(ts):.1f}) "
              f"over {len(ts)} alternating iterations after {args.warmup} warm-up")
    print(f"peak device memory with both models resident: {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="+", choices=["loop", "gather", "iter"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    print("build", build.source_fingerprint(), "device", torch.cuda.get_device_name(0))
    if "loop" in a.what or "gather" in a.what:
        loop_and_gather(a, a.what)
        torch.cuda.empty_cache()
    if "iter" in a.what:
        iteration(a)
