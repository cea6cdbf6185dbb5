"""Numbers behind profiles/train_image_pipeline.txt (one MI355X):

  errors  the train-mode image kernels at seed 18 against golden F18 and against the torch-CPU restatement
          (tests/train_pipeline_ref.py): maximum and mean absolute error for frames, depth and segmentation maps
  time    one B = 8 call of TrainImagePipeline (64 frames in one launch + 32 depth + 32 segmentation maps in one launch each):
          device events around repeated calls after a warm-up, median with the spread; next to it the bytes of reading every
          input once and writing every output once, and the host time of the restatement on the same inputs

    python tools/measure_train_image_pipeline.py errors time
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_pipeline_ref as R  # noqa: E402
from thinktwice_amd import build, calib, synth  # noqa: E402
from thinktwice_amd.preprocess import IdaSampler, TrainImagePipeline  # noqa: E402


def errors(pipe):
    raw, depth, seg, params, ref = R.seed18()
    out = pipe(torch.from_numpy(raw)[None].cuda(), torch.from_numpy(depth)[None].cuda(), torch.from_numpy(seg)[None].cuda(),
               sampler=IdaSampler(calib.IDA_AUG_CONF, 18))
    assert out["params"] == [params]
    got = {k: out[k][0].cpu() for k in ("img", "depth", "seg")}
    e = R.errors_against_f18(*(got[k].numpy() for k in ("img", "depth", "seg")))
    print("seed 18, against golden F18 (sampled values, one row and one column per image) and against the restatement (every pixel)")
    for k, unit in (("img", "normalised units"), ("depth", "m"), ("seg", "class ids")):
        d = (got[k] - ref[k]).abs()
        print(f"  {k:5s} vs F18: max {e[k][0]:.3e} mean {e[k][1]:.3e}   vs restatement: max {float(d.max()):.3e} "
              f"mean {float(d.mean()):.3e}   ({unit})")


def timing(pipe, B, repeats):
    T, N, H, W = 2, 4, calib.IMG_H, calib.IMG_W
    fh, fw = pipe.final_dim
    raws, deps, segs = [], [], []
    for b in range(B):
        raws.append(synth.raw_camera_frames(100 + b))
        d, s = synth.raw_label_maps(100 + b)
        deps.append(d)
        segs.append(s)
    raw, depth, seg = (torch.from_numpy(np.stack(x)).cuda() for x in (raws, deps, segs))
    params = IdaSampler(calib.IDA_AUG_CONF, 7).sample(B, N)
    fn = lambda: pipe(raw, depth, seg, params=params)   # noqa: E731
    for _ in range(3):
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
    med = statistics.median(ms)
    rd = raw.numel() + 4 * (depth.numel() + seg.numel()) + 2 * 4 * H * W
    wr = 4 * (B * T * N * 3 * fh * fw + 2 * B * N * fh * fw)
    print(f"B = {B}: {B * T * N} frames + {B * N} depth + {B * N} segmentation maps, 3 launches, NCHW f32 output")
    print(f"  device time of one call: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) over {repeats} calls after 3 warm-up")
    print(f"  every input read once {rd / 1e6:.1f} MB + every output written once {wr / 1e6:.1f} MB = {(rd + wr) / 1e6:.1f} MB "
          f"-> {(rd + wr) / med / 1e6:.1f} GB/s achieved")
    mx, my = calib.undistort_rectify_map()
    t0 = time.perf_counter()
    for b in range(B):
        R.restate(raws[b], params[b], mx, my, deps[b], segs[b])
    print(f"  torch-CPU restatement of the same {B} samples: {time.perf_counter() - t0:.2f} s on {torch.get_num_threads()} threads "
          f"(host clock, one pass)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="+", choices=["errors", "time"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured on the host")
    print("build", build.source_fingerprint(), "device", torch.cuda.get_device_name(0))
    pipe = TrainImagePipeline(calib.IDA_AUG_CONF)
    if "errors" in a.what:
        errors(pipe)
    if "time" in a.what:
        timing(pipe, a.batch, a.repeats)
