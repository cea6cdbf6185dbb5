"""Numbers behind profiles/eval_metrics.txt (one MI355X): what the device task metrics of thinktwice_amd/evaluate.py cost, at the
thinktwice.py size, B = 8, on bench_loader's generated dataset, in one process, the variants alternating with an A/A pair.

    python -m thinktwice_amd.bench_eval [--batch 8] [--rounds 3] [--out profiles/eval_metrics.txt]

  1. `forward_inference` alone (x, x') against `forward_inference` + `MetricWindow.add` (y), `--forwards` calls per leg on one
     batch, each leg between two device synchronises on the host clock;
  2. a validation pass, `runner.validate`, with `metrics` off (x, x': the code path of a build without the feature) against
     `metrics` on (y), one pass over the loader per leg;
  3. each kernel of csrc/eval_metrics.hip between two device events, and the bytes per second it achieves against its compulsory
     bytes (every input byte it has to read once).
They are recorded as information, not as pass criteria; the structural condition -- `add` adds no host synchronisation -- is
tests/test_evaluate.py's."""
import argparse
import os
import shutil
import statistics
import tempfile
import time

from . import bench_loader, build, calib


def _measure(root, metadata, B, rounds, forwards, emit):
    import torch
    from . import dataset, evaluate, model as tm, params
    from ._lib import check, cur_stream, lib, ptr
    from .loader import DeviceBatchLoader
    from .runner import validate
    from .trainer import Trainer
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured on the host alone")
    emit(f"build {build.source_fingerprint()} device {torch.cuda.get_device_name(0)}")
    sync, med = torch.cuda.synchronize, statistics.median
    index = dataset.DatasetIndex(metadata, ["town01_00"], bench_loader.CFG, root=root)
    loader = DeviceBatchLoader(index, bench_loader.CFG, calib.IDA_AUG_CONF, batch_size=B, seed=1, prefetch=2, threads=8, train=False,
                               png=dict(verify=("adler32",), segments="require"))
    n = len(loader)
    model, cfg = tm.build_thinktwice(dtype="f32x3", device="cuda")
    trainer = Trainer(model, params.init_params(cfg, seed=0), frozen_bn=False)
    model.eval()
    batch = None
    for b in loader:                                                      # (a whole pass; its first batch is measurement 1's)
        batch = b if batch is None else batch
    window = evaluate.window_for(model)

    def fwd():
        for _ in range(forwards):
            model.forward_inference(batch)

    def fwd_add():
        for _ in range(forwards):
            window.add(batch, model.forward_inference(batch))

    def leg(fn, per):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3 / per

    def rounds_of(x_fn, y_fn, per):
        x1, x2, y = [], [], []
        for _ in range(rounds):
            x1.append(leg(x_fn, per))
            x2.append(leg(x_fn, per))
            y.append(leg(y_fn, per))
        return x1, x2, y

    def report(what_x, what_y, unit, x1, x2, y):
        x, spread = med(x1 + x2), abs(med(x1) - med(x2))
        emit(f"  (x) {what_x}: {x:8.2f} ms per {unit} (x {med(x1):.2f}, x' {med(x2):.2f}: A/A spread {spread:.2f} ms; min "
             f"{min(x1 + x2):.2f}, max {max(x1 + x2):.2f}, n = {len(x1 + x2)})")
        emit(f"  (y) {what_y}: {med(y):8.2f} ms per {unit} (min {min(y):.2f}, max {max(y):.2f}, n = {len(y)}); (y) - (x) = "
             f"{med(y) - x:+.2f} ms")

    with torch.no_grad():
        fwd_add()                                                         # warm-up: allocator, first launches, both paths
        sync()
        emit(f"B = {B}, thinktwice.py size, f32x3, eval(); {rounds} rounds of [x, x', y]; host clock, a device synchronise before and "
             f"after every leg; medians")
        emit(f"1. forward_inference, {forwards} calls per leg on one batch")
        report("forward_inference alone", "forward_inference + MetricWindow.add", "call", *rounds_of(fwd, fwd_add, forwards))
    window.close()

    def val_off():
        validate(trainer, loader)

    def val_on():
        validate(trainer, loader, metrics=evaluate.window_for(model))

    val_on()
    emit(f"2. runner.validate over the loader ({n} batches of {B}; forward_train under eval(), prefetch = 2), one pass per leg")
    report("metrics off (the code path without the feature)", "metrics on (MetricWindow filled from the same forwards)", "batch",
           *rounds_of(val_off, val_on, n))
    loader.close()

    # ---- the kernels, device events around back-to-back launches
    dev, st, L = model.device, cur_stream(model.device), lib()
    with torch.no_grad():
        pred = model.forward_inference(batch)
    seg, dep = pred["_seg_cl"].float().contiguous(), pred["_depth_cl"].float().contiguous()
    lab, gt = batch["seg"].float().contiguous(), batch["depth"].float().contiguous()
    acc = torch.zeros(4096, dtype=torch.int64, device=dev)
    facc = acc.view(torch.float64)

    def events(fn, reps=20):
        fn()
        sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    b_, n_, H, W = lab.shape
    fs, fd, db = model.seg_downsample_factor, model.downsample_factor, model.d_bound
    Dn = int((db[1] - db[0]) / db[2])
    cells_s, cells_d = b_ * n_ * (H // fs) * (W // fs), b_ * n_ * (H // fd) * (W // fd)
    rows = []
    t = events(lambda: check(L.tt_eval_seg_confusion(ptr(seg), seg.shape[-1], 12, ptr(lab), b_ * n_, H, W, fs, ptr(acc), st), "seg"))
    # the 12 class channels of a cell (three 16-byte pieces) and its one 4-byte label
    rows.append(("tt_eval_seg_confusion", t, cells_s * (12 * 4 + 4), f"{cells_s} cells, pitch {seg.shape[-1]}"))
    t = events(lambda: check(L.tt_eval_depth_bins(ptr(dep), dep.shape[-1], Dn, ptr(gt), b_ * n_, H, W, fd, db[0], db[2], ptr(acc), st),
                             "depth"))
    rows.append(("tt_eval_depth_bins", t, gt.numel() * 4 + cells_d * Dn * 4, f"{cells_d} cells of {fd} x {fd} pixels, {Dn} bins (the "
                 f"logits of background cells are not read: the figure counts them, so it is an upper bound on the bytes)"))
    wp, mu, sg, sp = (pred[k].float().contiguous() for k in ("pred_wp", "mu_branches", "sigma_branches", "pred_speed"))
    gw, gm, gs, gv = (batch[k].float().contiguous() for k in ("waypoints", "action_mu", "action_sigma", "speed"))
    t = events(lambda: check(L.tt_eval_decoder(ptr(wp), ptr(mu), ptr(sg), ptr(sp), ptr(gw), ptr(gm), ptr(gs), ptr(gv), wp.shape[0],
                                               wp.shape[1], ptr(facc[1024:]), ptr(acc[2048:]), st), "decoder"))
    rows.append(("tt_eval_decoder", t, sum(x.numel() for x in (wp, mu, sg, sp, gw, gm, gs, gv)) * 4, f"B = {wp.shape[0]}, one "
                 f"64-thread workgroup, latency-bound"))
    seg_b = seg.clone()
    t = events(lambda: check(L.tt_eval_pair_deviation(ptr(seg), ptr(seg_b), seg.numel(), ptr(acc[3000:]), st), "pair"))
    rows.append(("tt_eval_pair_deviation", t, 2 * seg.numel() * 4, f"two seg maps of {seg.numel()} floats"))
    t = events(lambda: check(L.tt_eval_pair_seg(ptr(seg), ptr(seg_b), seg.shape[-1], 12, cells_s, ptr(acc[3100:]), st), "pair_seg"))
    rows.append(("tt_eval_pair_seg", t, 2 * cells_s * 12 * 4, f"{cells_s} cells"))
    t = events(lambda: check(L.tt_eval_pair_wp(ptr(wp), ptr(wp), wp.numel() // 2, ptr(facc[3200:]), ptr(acc[3300:]), st), "pair_wp"))
    rows.append(("tt_eval_pair_wp", t, 2 * wp.numel() * 4, f"{wp.numel() // 2} points, one 64-thread workgroup, latency-bound"))
    emit("3. kernels, 20 back-to-back launches between two device events, us per launch INCLUDING the launch gap; compulsory bytes = "
         "every input byte the kernel has to read once")
    for name, us, nbytes, note in rows:
        emit(f"  {name:24s} {us:9.1f} us, {nbytes / 1e6:9.3f} MB compulsory, {nbytes / us / 1e3:8.1f} GB/s  ({note})")


def main(B, rounds, forwards, emit):
    tmp = tempfile.mkdtemp(prefix="tt_bench_eval_data_")
    try:
        root, metadata, _, _, writer = bench_loader.write_dataset(tmp, B)
        emit(f"dataset: bench_loader's (one route of {B + 5} frames under {bench_loader.LINKS} names, PNG files written by {writer}, "
             f"segmented at R = {bench_loader.ROWS})")
        _measure(root, metadata, B, rounds, forwards, emit)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--forwards", type=int, default=5, help="forward_inference calls per leg of measurement 1")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    main(args.batch, args.rounds, args.forwards, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
