"""Numbers behind profiles/train_runner.txt (one MI355X): runner.EpochRunner against the hand loop it replaces, at the
thinktwice.py size, B = 8, on bench_loader's generated dataset (twelve batches per epoch, files in the page cache), prefetch = 2.

    python -m thinktwice_amd.bench_runner [--batch 8] [--rounds 3] [--out profiles/train_runner.txt]

Two loops alternate in one process over the same loader and trainer, one epoch per leg, each leg between two device
synchronises on the host clock:
  (x) for batch in loader: trainer.step(batch)        the float log_vars and the finite check: two host waits per iteration
  (y) EpochRunner's epoch, log_interval = 4           trainer.step(batch, check_finite=False, device_log=True) + LogWindow
Per round the order is x, x', y: (x) against (x') is the A/A spread.  Reported per iteration: the whole epoch / 12 (this is
what the condition is about: (y) not slower than (x) by more than the A/A spread), and the steady-state hand-over interval
(iterations 3..10 of the epoch, from the loader's hand-over times).  Then the three logvars kernels from device events, and
the number of torch operators parse_losses dispatches with and without device_log on a dict of the real one's shapes.

    python -m thinktwice_amd.bench_runner --cumulative-iters 1 2 4 [--out profiles/train_accumulate.txt]

measures gradient accumulation instead (profiles/train_accumulate.txt): EpochRunner's epoch under every given cumulative_iters,
one runner per k over the same loader and trainer, per round the legs [k = 1, k = 1 again, then the other k]; ms per
micro-iteration (the epoch / 12), and k = 1 against its repeat as the A/A spread.  With `--cumulative-iters 1` alone it uses
nothing a build without accumulation lacks, which is how the parent commit's leg is measured beside it."""
import argparse
import os
import shutil
import statistics
import tempfile
import time

from . import bench_loader, build, calib


class _Timed:
    """The loader, noting the host time of every hand-over."""

    def __init__(self, loader):
        self.loader, self.times = loader, []

    def __len__(self):
        return len(self.loader)

    def set_epoch(self, e):
        self.loader.set_epoch(e)

    def __iter__(self):
        self.times = []
        for batch in self.loader:
            self.times.append(time.perf_counter())
            yield batch


def _count_ops(fn):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Count.n += 1
            return func(*args, **(kwargs or {}))

    with Count():
        fn()
    return Count.n


def _measure(root, metadata, B, rounds, emit):
    import torch
    from . import dataset, logvars, losses as LS, model as tm, params
    from ._lib import check, cur_stream, lib, ptr
    from .loader import DeviceBatchLoader
    from .runner import EpochRunner
    from .trainer import Trainer
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured on the host alone")
    emit(f"build {build.source_fingerprint()} device {torch.cuda.get_device_name(0)}")
    sync, med = torch.cuda.synchronize, statistics.median
    index = dataset.DatasetIndex(metadata, ["town01_00"], bench_loader.CFG, root=root)
    n = bench_loader.LINKS
    loader = _Timed(DeviceBatchLoader(index, bench_loader.CFG, calib.IDA_AUG_CONF, batch_size=B, seed=1, prefetch=2, threads=8,
                                      png=dict(verify=("adler32",), segments="require")))
    model, cfg = tm.build_thinktwice(dtype="f32x3", device="cuda")
    trainer = Trainer(model, params.init_params(cfg, seed=0), frozen_bn=False)
    work = tempfile.mkdtemp(prefix="tt_bench_runner_")
    runner = EpochRunner(trainer, loader, work_dir=work, max_epochs=10 ** 6, log_interval=4, verbose=False)
    trainer.set_schedule(10 ** 6 * n, n)

    def hand(e):
        loader.set_epoch(e)
        for batch in loader:
            trainer.step(batch)

    def leg(fn, e):
        sync()
        t0 = time.perf_counter()
        fn(e)
        sync()
        whole = (time.perf_counter() - t0) * 1e3 / n
        t = loader.times
        return whole, (t[n - 2] - t[2]) * 1e3 / (n - 4)

    hand(0)                                                              # warm-up: allocator, first launches, both paths
    runner._train_epoch(1)
    sync()
    x1, x2, y, sx, sy = [], [], [], [], []
    e = 2
    for _ in range(rounds):
        for store, steady, fn in ((x1, sx, hand), (x2, sx, hand), (y, sy, runner._train_epoch)):
            w, s = leg(fn, e)
            store.append(w)
            steady.append(s)
            e += 1
    loader.loader.close()
    shutil.rmtree(work, ignore_errors=True)
    x, spread = med(x1 + x2), abs(med(x1) - med(x2))
    emit(f"B = {B}, thinktwice.py size, f32x3, frozen_bn=False, prefetch = 2, {n} iterations per epoch, {rounds} rounds of "
         f"[x, x', y], one epoch per leg; host clock, a device synchronise before and after every leg; medians")
    emit(f"  (x) for batch in loader: trainer.step(batch):   {x:8.1f} ms per iteration over the epoch (x {med(x1):.1f}, x' {med(x2):.1f}: "
         f"A/A spread {spread:.1f} ms; min {min(x1 + x2):.1f}, max {max(x1 + x2):.1f}, n = {len(x1 + x2)}); steady-state hand-over "
         f"interval {med(sx):.1f} ms")
    emit(f"  (y) EpochRunner, log_interval = 4:              {med(y):8.1f} ms per iteration over the epoch (min {min(y):.1f}, max {max(y):.1f}, "
         f"n = {len(y)}); steady-state hand-over interval {med(sy):.1f} ms")
    emit(f"  (y) - (x) = {med(y) - x:+.1f} ms per iteration; the condition -- (y) not slower than (x) by more than the A/A spread of "
         f"(x), {spread:.1f} ms -- is {'met' if med(y) - x <= spread else 'NOT met'}")
    emit(f"  log lines written by (y): {len(runner.logs)} ({n // 4} per epoch), none of them waited for inside an iteration "
         f"except at the end of an epoch")

    # ---- the three kernels, device events around 50 back-to-back launches each
    dev = model.device
    names = tuple(f"t{i}_loss" for i in range(23))
    terms = {k: torch.rand((), device=dev) for k in names}
    st = cur_stream(dev)

    def events(fn, reps=50):
        fn()
        sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    _, packed, _ = logvars.pack(terms)
    window = torch.zeros(24 + 1 + 3, dtype=torch.float64, device=dev)
    out = torch.empty_like(window)
    norm = torch.ones(2, device=dev)
    t_pack = events(lambda: logvars.pack(terms))
    t_acc = events(lambda: check(lib().tt_logvars_accumulate(ptr(packed), 24, ptr(norm), 1, B, ptr(norm), ptr(window), st), "acc"))
    t_flush = events(lambda: check(lib().tt_logvars_flush(ptr(window), 28, ptr(out), st), "flush"))
    emit(f"  kernels, 50 back-to-back launches between two device events, us per launch INCLUDING the launch gap (each kernel is "
         f"one 64-thread workgroup): tt_logvars_pack (23 terms, called through logvars.pack: the host's table fill and the output's "
         f"allocation are inside the figure, which is host-bound) {t_pack:.1f}, tt_logvars_accumulate (24 + 1 values) {t_acc:.1f}, "
         f"tt_logvars_flush (28 doubles) {t_flush:.1f}")

    # ---- torch operators parse_losses dispatches (each is one kernel launch or copy on the device)
    real = dict(terms)
    real["t6_loss"] = torch.rand((B, 1), device=dev)                      # value_loss is (B, 1): reduced by its own .mean()
    a = _count_ops(lambda: LS.parse_losses(real))
    b = _count_ops(lambda: LS.parse_losses(real, device_log=True))
    emit(f"  torch operators dispatched by parse_losses on a dict of the real one's shapes (22 scalars and one (B, 1) term): "
         f"{a} without device_log (mean / add / stack per name, one device-to-host copy that waits), {b} with it (the (B, 1) "
         f"term's mean, the output's allocation; then ONE launch of tt_logvars_pack, no copy)")
    emit("  not run with two real ranks: the cross-rank merge of a validation and the all-reduce of the packed vector are covered "
         "by the arithmetic tests only (tests/test_runner_cpu.py)")


def _measure_accumulate(root, metadata, B, rounds, ks, emit):
    import torch
    from . import dataset, model as tm, params
    from .loader import DeviceBatchLoader
    from .runner import EpochRunner
    from .trainer import Trainer
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured on the host alone")
    emit(f"build {build.source_fingerprint()} device {torch.cuda.get_device_name(0)}")
    sync, med = torch.cuda.synchronize, statistics.median
    index = dataset.DatasetIndex(metadata, ["town01_00"], bench_loader.CFG, root=root)
    n = bench_loader.LINKS
    loader = DeviceBatchLoader(index, bench_loader.CFG, calib.IDA_AUG_CONF, batch_size=B, seed=1, prefetch=2, threads=8,
                               png=dict(verify=("adler32",), segments="require"))
    model, cfg = tm.build_thinktwice(dtype="f32x3", device="cuda")
    trainer = Trainer(model, params.init_params(cfg, seed=0), frozen_bn=False)
    trainer.set_schedule(10 ** 6 * n, n)
    works, runners = [], {}
    for k in ks:
        works.append(tempfile.mkdtemp(prefix="tt_bench_runner_"))
        runners[k] = EpochRunner(trainer, loader, work_dir=works[-1], max_epochs=10 ** 6, log_interval=4, verbose=False,
                                 **({"cumulative_iters": k} if k > 1 else {}))
    legs = [(1, "a"), (1, "b")] + [(k, "a") for k in ks if k != 1]          # per round: k = 1, its repeat, the others
    times = {leg: [] for leg in legs}
    e = 0
    for k in ks:                                                           # warm-up: allocator, first launches, every path
        runners[k]._train_epoch(e)
        e += 1
    sync()
    for _ in range(rounds):
        for leg in legs:
            sync()
            t0 = time.perf_counter()
            runners[leg[0]]._train_epoch(e)
            sync()
            times[leg].append((time.perf_counter() - t0) * 1e3 / n)
            e += 1
    trainer.reconcile()
    loader.close()
    for w in works:
        shutil.rmtree(w, ignore_errors=True)
    a, b = times[1, "a"], times[1, "b"]
    base, spread = med(a + b), abs(med(a) - med(b))
    emit(f"B = {B}, thinktwice.py size, f32x3, frozen_bn=False, prefetch = 2, {n} iterations per epoch, log_interval = 4, {rounds} "
         f"rounds of [{', '.join(f'k = {k}' + chr(39) * (tag == 'b') for k, tag in legs)}], one epoch of EpochRunner per leg; host "
         f"clock, a device synchronise before and after every leg; medians, ms per MICRO-iteration over the epoch")
    emit(f"  cumulative_iters = 1 (plain steps):   {base:8.1f} ms (k = 1 {med(a):.1f}, k = 1' {med(b):.1f}: A/A spread {spread:.1f} ms; "
         f"min {min(a + b):.1f}, max {max(a + b):.1f}, n = {len(a + b)})")
    for k in ks:
        if k == 1:
            continue
        t = times[k, "a"]
        emit(f"  cumulative_iters = {k} ({n // k} updates per epoch): {med(t):8.1f} ms (min {min(t):.1f}, max {max(t):.1f}, n = {len(t)}); "
             f"{med(t) - base:+.1f} ms against k = 1 beside it")
    emit(f"  skipped updates found by reconcile() over the whole run: {trainer.opt.skipped()}")
    return base, spread, {k: med(times[k, "a"]) for k in ks if k != 1}


def main(B, rounds, emit, cumulative_iters=None):
    tmp = tempfile.mkdtemp(prefix="tt_bench_runner_data_")
    try:
        root, metadata, _, _, writer = bench_loader.write_dataset(tmp, B)
        emit(f"dataset: bench_loader's (one route of {B + 5} frames under {bench_loader.LINKS} names, PNG files written by {writer}, "
             f"segmented at R = {bench_loader.ROWS})")
        if cumulative_iters:
            _measure_accumulate(root, metadata, B, rounds, sorted(set([1] + list(cumulative_iters))), emit)
            return
        _measure(root, metadata, B, rounds, emit)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--cumulative-iters", type=int, nargs="+", default=None, metavar="K", help="measure EpochRunner under these "
                    "cumulative_iters instead (k = 1 is always measured, twice per round)")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    main(args.batch, args.rounds, emit, args.cumulative_iters)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
