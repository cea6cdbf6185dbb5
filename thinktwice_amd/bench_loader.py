"""Numbers behind profiles/train_loader.txt (one MI355X): loader.DeviceBatchLoader feeding trainer.Trainer.step at the
thinktwice.py size, B = 8, from segmented files (R = 16) with verify=("adler32",).

    python -m thinktwice_amd.bench_loader [--batch 8] [--rounds 2] [--out profiles/train_loader.txt]

The dataset is written into a temporary directory first, by forked processes, before this process touches the device: one
route of B + 5 frames of 900 x 1600 (camera frames and tags of synth.raw_label_bytes, depth maps a smooth ramp in CARLA's
24-bit code, as bench_png.py makes them; written by PIL when it is importable, else by tests/png_cases.py; then
png.segment_png at R = 16), LiDAR sweeps of 65,536 points, measurement and supervision files of the dataset's shapes.  The
route has B samples; it appears under twelve names (symbolic links), so an epoch has twelve batches whose files the page
cache holds: what is measured is the loader and the device, not the disk.

Three cases alternate in one process, each iteration closed by a device synchronise and timed on the host clock:
  (a) the loader alone, prefetch = 0: ms per batch, with its parts -- the reader threads (files + frame_info), the
      coordinating thread's pack and launches, the device's time from the first launch to the last (events on the side
      stream), and a pinned host-to-device copy of as many bytes as the batch uploads, timed on its own;
  (b) Trainer.step on a resident loader batch, twice per round (A/A): the `train_step` leg's quantity;
  (c) for batch in loader: trainer.step(batch), prefetch = 2, in steady state: the iterations that queue a later batch's
      stages and train on one queued two iterations earlier.  The first two iterations of an epoch, which fill the
      pipeline, and the last two, which queue nothing, are reported apart.
What must hold: (c) < (a) + (b) by more than the A/A spread of (b)."""
import argparse
import json
import multiprocessing
import os
import pickle
import shutil
import statistics
import tempfile
import time

import numpy as np

from . import bench_png, build, calib, synth
from .bench_forward import TORCH_DTYPE

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
H, W, N = 900, 1600, 4
ROWS = 16
LINKS = 12
GRID_SHAPES = [(1,), (1,), (32, 21, 21), (64, 10, 10), (128, 4, 4), (256, 2, 2)]
CFG = {"pred_len": 4, "history_query_index_lis": [-1, 0], "is_local": True, "is_full": True, "max_sample_per_town": {"town01": 1e9},
       "camera_names": list(calib.CAMERA_NAMES), "seg_label_idxs": [1, 4, 5, 6, 7, 8, 10, 12, 18]}
_ROUTE = [None]


def _write_frame(f):
    """One frame's files (a forked worker: no GPU)."""
    from . import png
    write, _ = bench_png._writer()
    route = _ROUTE[0]
    rng = np.random.default_rng(500 + f)
    _, tags, rgb = synth.raw_label_bytes(200 + f, N, H, W)
    sizes = [0, 0]
    for n, cam in enumerate(calib.CAMERA_NAMES):
        for kind, a in (("rgb", rgb[n]), ("depth", bench_png._depth_ramp(4 * f + n)), ("seg", tags[n])):
            plain = write(np.ascontiguousarray(a))
            data = png.segment_png(plain, ROWS)
            sizes[0] += len(plain)
            sizes[1] += len(data)
            with open(os.path.join(route, cam.replace("rgb", kind), f"{f:04d}.png"), "wb") as fh:
                fh.write(data)
    p = np.empty((65536, 4), np.float32)
    p[:, 0], p[:, 1] = rng.uniform(-8, 30.4, 65536), rng.uniform(-19.2, 19.2, 65536)
    p[:, 2], p[:, 3] = rng.uniform(-4, 4, 65536), rng.uniform(0, 1, 65536)
    np.save(os.path.join(route, "lidar", f"{f:04d}.npy"), p)
    meas = {"x": 100.0 + 0.9 * f + 0.05 * rng.normal(), "y": -40.0 + 0.3 * f + 0.05 * rng.normal(), "theta": 0.3 + 0.01 * f,
            "speed": float(rng.uniform(2, 8)), "x_target": 130.0, "y_target": -30.0, "target_command": 1 + f % 6,
            "acceleration": rng.normal(size=3).tolist(), "angular_velocity": (0.1 * rng.normal(size=3)).tolist()}
    with open(os.path.join(route, "measurements", f"{f:04d}.json"), "w") as fh:
        json.dump(meas, fh)
    f32 = lambda a: np.asarray(a, np.float32)                                   # noqa: E731
    sup = {"action": f32(rng.uniform(-1, 1, 3)), "action_mu": f32(rng.uniform(0.5, 4, 2)), "action_sigma": f32(rng.uniform(0.5, 4, 2)),
           "only_ap_brake": f % 3 == 0, "value": np.float32(rng.normal()), "features": f32(rng.normal(size=256)),
           "cnn_features": [f32(rng.normal(size=s)) for s in GRID_SHAPES]}
    np.save(os.path.join(route, "supervision", f"{f:04d}.npy"), np.array(sup, dtype=object), allow_pickle=True)
    return sizes


def write_dataset(tmp, B):
    """-> (root, metadata path, plain file bytes, segmented file bytes, writer name)."""
    data_dir = os.path.join(tmp, "dataset", "town01_00")
    route = os.path.join(data_dir, "routes_0")
    for k in ["measurements", "supervision", "lidar"] + [c.replace("rgb", k) for k in ("rgb", "depth", "seg") for c in calib.CAMERA_NAMES]:
        os.makedirs(os.path.join(route, k))
    os.makedirs(os.path.join(tmp, "work"))
    _ROUTE[0] = route
    L = B + 5
    with multiprocessing.get_context("fork").Pool(min(L, 16)) as pool:           # before this process touches the device
        sizes = pool.map(_write_frame, range(L), chunksize=1)
    metadata = {"town01_00": {"../town01_00/routes_0": L}}
    for k in range(1, LINKS):
        os.symlink(route, os.path.join(data_dir, f"routes_{k}"))
        metadata["town01_00"][f"../town01_00/routes_{k}"] = L
    path = os.path.join(tmp, "dataset", "dataset_metadata.pkl")
    with open(path, "wb") as fh:
        pickle.dump(metadata, fh)
    return os.path.join(tmp, "work"), path, sum(s[0] for s in sizes), sum(s[1] for s in sizes), bench_png._writer()[1]


def main(B, rounds, emit):
    tmp = tempfile.mkdtemp(prefix="tt_bench_loader_")
    try:
        t0 = time.perf_counter()
        root, metadata, plain_bytes, seg_bytes, writer = write_dataset(tmp, B)
        emit(f"dataset: one route of {B + 5} frames under {LINKS} names ({B * LINKS} samples, {LINKS} batches of {B} per epoch), "
             f"{(B + 5) * 12} PNG files of {H} x {W} written by {writer}, segmented at R = {ROWS} ({seg_bytes} file bytes, "
             f"{seg_bytes / plain_bytes:.3f} x the unsegmented), made in {time.perf_counter() - t0:.0f} s by forked host processes")
        _measure(root, metadata, B, rounds, emit)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _measure(root, metadata, B, rounds, emit):
    import torch
    from . import dataset, model as tm, params
    from .loader import DeviceBatchLoader
    from .trainer import Trainer
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured on the host alone")
    emit(f"build {build.source_fingerprint()} device {torch.cuda.get_device_name(0)}")
    index = dataset.DatasetIndex(metadata, ["town01_00"], CFG, root=root)
    assert len(index) == B * LINKS
    png_args = dict(verify=("adler32",), segments="require")
    sync = torch.cuda.synchronize

    # ---- the loader alone first: its memory, before the model is there
    alone = DeviceBatchLoader(index, CFG, calib.IDA_AUG_CONF, batch_size=B, seed=0, prefetch=0, threads=8, png=png_args)
    it = iter(alone)
    resident = next(it)                                                          # (warm-up: allocator, kernels' first launch)
    sync()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    held = next(it)
    sync()
    peak, after = torch.cuda.max_memory_allocated() - base, torch.cuda.memory_allocated() - base
    del held
    alone.close()
    emit(f"device memory of one in-flight slot, B = {B}: peak {peak / 2 ** 20:.0f} MiB above the resting level while the batch "
         f"is built (decoded frames, the label decoder's workspace), {after / 2 ** 20:.0f} MiB once it is handed over "
         f"(img, depth, seg, points, targets); with prefetch = p up to p + 1 batches are held and one is being built")

    model, cfg = tm.build_thinktwice(dtype=TORCH_DTYPE["bf16x3"], device="cuda")
    trainer = Trainer(model, params.init_params(cfg, seed=0), frozen_bn=False)
    for _ in range(2):
        out = trainer.step(resident, check_finite=False)
    sync()
    emit(f"Trainer.step(frozen_bn=False, f32x3) on a loader batch: loss {float(out['loss']):.4f}, "
         f"gradient norm {float(out['grad_norm'][0]):.3f}")
    ahead = DeviceBatchLoader(index, CFG, calib.IDA_AUG_CONF, batch_size=B, seed=1, prefetch=2, threads=8, png=png_args)

    a_ms, a_parts, b1, b2, c_ms, c_fill, c_drain = [], [], [], [], [], [], []
    for r in range(rounds):
        alone.set_epoch(r)
        sync()
        t0 = time.perf_counter()
        for k, batch in enumerate(alone):                                        # (a)
            sync()
            t1 = time.perf_counter()
            if k:                                                                # (the epoch's first batch starts the threads)
                a_ms.append((t1 - t0) * 1e3)
                a_parts.append(dict(alone.last["timings"]))
            del batch
            t0 = time.perf_counter()
        for store in (b1, b2):                                                   # (b), A/A
            for _ in range(4):
                sync()
                t0 = time.perf_counter()
                trainer.step(resident, check_finite=False)
                sync()
                store.append((time.perf_counter() - t0) * 1e3)
        ahead.set_epoch(r)
        sync()
        t0 = time.perf_counter()
        for k, batch in enumerate(ahead):                                        # (c)
            trainer.step(batch, check_finite=False)
            sync()
            t1 = time.perf_counter()
            (c_fill if k < 2 else c_drain if k >= LINKS - 2 else c_ms).append((t1 - t0) * 1e3)
            del batch
            t0 = time.perf_counter()
    alone.close()
    ahead.close()

    up = int(statistics.median(p["png_packed_bytes"] + p["cloud_bytes"] + p["target_bytes"] for p in a_parts))
    src, dst = torch.empty(up, dtype=torch.uint8, pin_memory=True), torch.empty(up, dtype=torch.uint8, device="cuda")
    ups = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        e1.synchronize()
        ups.append(e0.elapsed_time(e1))
    med = statistics.median
    a, b_1, b_2, c = med(a_ms), med(b1), med(b2), med(c_ms)
    b, spread = med(b1 + b2), abs(b_1 - b_2)
    part = lambda k, s=1e3: med(p[k] * s for p in a_parts)                      # noqa: E731
    emit(f"B = {B}, thinktwice.py size, {rounds} rounds of [(a) {LINKS - 1} batches, (b) 2 x 4 steps, (c) {LINKS - 4} steady "
         f"iterations] alternating in one process; host clock around iterations closed by a device synchronise; medians")
    emit(f"  (a) loader alone, prefetch = 0, threads = 8:          {a:8.1f} ms per batch (min {min(a_ms):.1f}, max {max(a_ms):.1f}, n = {len(a_ms)})")
    emit(f"        reader threads: files + frame_info + clouds     {part('read_wait_s'):8.1f} ms (the slowest sample's own time {part('read_s'):.1f} ms)")
    emit(f"        coordinating thread: draws, pack, launches      {part('launch_s'):8.1f} ms")
    emit("          of which inside the stages' calls: " + ", ".join(
        f"{k} {med(p['host_stage_s'][k] * 1e3 for p in a_parts):.1f} ms" for k in ("png", "labels", "pipeline", "union", "targets"))
        + " (png: chunk walk, the one host copy of the streams into the pinned buffer, launches)")
    emit(f"        waiting for the device after the last launch    {part('event_wait_s'):8.1f} ms")
    emit(f"        device, first launch to last (side-stream events) {part('device_ms', 1):6.1f} ms: upload, inflate + unfilter + Adler-32, "
         f"labels, IDA + colour augmentation, sweep union")
    emit(f"        upload alone: {up} bytes (packed PNG streams, clouds, targets) as one pinned copy {med(ups):.2f} ms "
         f"({up / med(ups) / 1e6:.1f} GB/s)")
    emit(f"  (b) Trainer.step on a resident batch:                 {b:8.1f} ms (A {b_1:.1f}, A' {b_2:.1f}: A/A spread {spread:.1f} ms; "
         f"min {min(b1 + b2):.1f}, max {max(b1 + b2):.1f}, n = {len(b1 + b2)})")
    emit(f"  (c) for batch in loader: trainer.step(batch), prefetch = 2: {c:8.1f} ms per iteration in steady state "
         f"(min {min(c_ms):.1f}, max {max(c_ms):.1f}, n = {len(c_ms)}; the first two iterations of an epoch: {med(c_fill):.1f} ms, "
         f"the last two, which queue nothing: {med(c_drain):.1f} ms)")
    hidden = (a + b - c) / a
    emit(f"  serial sum (a) + (b) = {a + b:.1f} ms; (c) is {a + b - c:+.1f} ms below it: {100 * hidden:.0f} % of (a) is hidden "
         f"({'more' if a + b - c > spread else 'NOT more'} than the A/A spread of (b), {spread:.1f} ms); (c) - (b) = {c - b:+.1f} ms is what "
         f"the loader still costs an iteration")
    return {"a": a, "b": b, "c": c, "spread": spread, "hidden": hidden}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    main(args.batch, args.rounds, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
