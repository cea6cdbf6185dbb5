"""Numbers behind profiles/train_label_decode.txt (one MI355X): labels.RawLabelDecoder at B = 8, full size (32 depth PNGs, 32
tag maps and the 32 key-sweep frames of 900 x 1600, synth.raw_label_bytes), against the numpy / scipy restatement of the
reference's loader stage (tests/labels_ref.py) on the same images on the same box.

    python -m thinktwice_amd.bench_labels [--batch 8] [--repeats 30] [--out profiles/train_label_decode.txt]

Device events around each call after 3 warm-up rounds.  The phases of tt_decode_seg_u8 are separate launches inside one entry;
they are timed by difference: tt_decode_seg_u8_phases cuts the call short after phase k, the variants alternate in one process,
and phase k's time is median(0..k) - median(0..k-1).  Nothing here is measured on the host except the restatement."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

from . import build, labels, ops, synth
from .ops import check, lib, ptr

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SEG_LABEL_IDXS = [1, 4, 5, 6, 7, 8, 10, 12, 18]                 # configs/thinktwice.py:108
PHASES = ("tile (class map + local labels)", "edges (unions across tiles)", "flatten", "stats S (count, sum of S)",
          "stats HV (green, red)", "write")
ITERATION_MS = 750.0                                            # a training iteration at B = 8 (profiles/train_photometric.txt)


def _timed(fns, repeats):
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def main(B, repeats, threads, emit):
    N, H, W = 4, 900, 1600
    host = [synth.raw_label_bytes(200 + b, N, H, W) for b in range(B)]
    depth_np, tags_np, rgb_np = (np.stack([h[i] for h in host]) for i in range(3))
    raw = torch.from_numpy(rgb_np[:, None]).cuda()                # [B, T = 1, N, H, W, 3]: only the key sweep is read
    depth_u8, tags = torch.from_numpy(depth_np).cuda(), torch.from_numpy(tags_np).cuda()
    dec = labels.RawLabelDecoder(SEG_LABEL_IDXS)
    P = B * N * H * W
    need = labels.workspace_bytes(B * N, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(B, N, H, W, dtype=torch.float32, device="cuda")
    rgb = raw[:, -1]
    stream = ops.cur_stream(raw.device)

    def upto(k):
        check(lib().tt_decode_seg_u8_phases(ptr(tags), B, N, H, W, ptr(rgb), rgb.stride(0), ctypes.byref(dec.conf), ptr(ws), need,
                                            ptr(out), k, stream), "tt_decode_seg_u8_phases")

    fns = {"all": lambda: dec(raw, depth_u8, tags), "all'": lambda: dec(raw, depth_u8, tags),
           "depth": lambda: labels.decode_depth(depth_u8), "seg": lambda: labels.decode_seg(tags, rgb, dec.conf)}
    for k in range(6):
        fns[f"p{k}"] = lambda k=k: upto(k)
    ms = _timed(fns, repeats)
    med = {k: statistics.median(v) for k, v in ms.items()}
    lit = int((tags_np == 18).sum())
    emit(f"B = {B}: {B * N} images {H} x {W} (synth.raw_label_bytes(200 + b)); {lit} traffic-light pixels ({lit / P * 100:.2f} %); "
         f"device events around each call, {repeats} rounds after 3 warm-up rounds, the variants alternating in one process")
    for k, what in (("all", "RawLabelDecoder (depth + seg, workspace from torch's allocator)"), ("all'", "the same again (A/A)"),
                    ("depth", "decode_depth alone"), ("seg", "decode_seg alone")):
        emit(f"  {what:66s} median {med[k]:7.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})")
    spread = med["all'"] - med["all"]
    emit(f"  A/A spread: {spread:+.3f} ms")
    emit("  phases of tt_decode_seg_u8 by difference of cut-short calls (tt_decode_seg_u8_phases, a caller-held workspace):")
    prev = 0.0
    for k, what in enumerate(PHASES):
        emit(f"    {k}  {what:36s} {med[f'p{k}'] - prev:+8.3f} ms   (calls cut after it: median {med[f'p{k}']:.3f} ms)")
        prev = med[f"p{k}"]
    emit(f"  RawLabelDecoder / a {ITERATION_MS:.0f} ms training iteration at B = {B}: {med['all'] / ITERATION_MS * 100:.3f} %")
    emit(f"  workspace: {need} bytes ({need / 2 ** 20:.1f} MiB, 24 bytes per pixel)")
    emit(f"  host-to-device bytes per batch: f32 depth + f32 seg {8 * P} -> depth PNG bytes + tags {4 * P}: {4 * P} bytes "
         f"({4 * P / 1e6:.1f} MB) fewer; the RGB frames are on the device already")
    bytes_depth, bytes_tile = 3 * P + 4 * P, P + 4 * P
    emit(f"  bytes read + written once: decode_depth {bytes_depth / 1e6:.1f} MB -> {bytes_depth / med['depth'] / 1e6:.0f} GB/s; "
         f"tile phase {bytes_tile / 1e6:.1f} MB -> {bytes_tile / med['p0'] / 1e6:.0f} GB/s (an accounting, not a share of a measured peak)")

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import labels_ref as R
    torch.set_num_threads(threads)
    t0 = time.perf_counter()
    ref_seg = R.decode_seg_batch(tags_np, rgb_np, SEG_LABEL_IDXS)
    t1 = time.perf_counter()
    ref_depth = R.decode_depth(depth_np)
    t2 = time.perf_counter()
    depth, seg = dec(raw, depth_u8, tags)
    bad_seg = int((seg.cpu().numpy() != ref_seg).sum())
    bad_depth = int((depth.cpu().numpy().view(np.uint32) != ref_depth.view(np.uint32)).sum())
    emit(f"  tests/labels_ref.py on the same {B * N} images on this box, one process, {threads} thread(s) (numpy / scipy do not "
         f"thread these loops), host clock, one pass: LoadSeg {t1 - t0:.2f} s ({(t1 - t0) / (B * N) * 1e3:.0f} ms per image), "
         f"LoadDepth {t2 - t1:.2f} s")
    emit(f"  device against the restatement: {bad_seg} class ids and {bad_depth} depth values differ of {P} each")
    emit(f"  restatement / device: {(t2 - t0) * 1e3 / med['all']:.0f} x")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--threads", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured on the host")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"build {build.source_fingerprint()} device {torch.cuda.get_device_name(0)}")
    main(a.batch, a.repeats, a.threads, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
