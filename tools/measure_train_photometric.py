"""Numbers behind profiles/train_photometric.txt (one MI355X): the image call of TrainImagePipeline at B = 8, full size
(64 frames of 900 x 1600 -> 448 x 896, NCHW f32), without and with the colour augmentation of thinktwice_amd/photometric.py.

  a   pipe(raw, params=...)                           today's entry, tt_preprocess_images_ida (measured twice, a and a': A/A)
  b   augment = all-empty programs                    tt_preprocess_images_ida_aug, the uint8 truncation only
  c   augment = sampler programs at iteration 0       frequency 0.05: most samples get nothing
  d   augment = sampler programs at iteration 1.5e6   all eight operators and a blur on every sample (two launches + scratch)

Device events around each call, 3 warm-up rounds, then `--repeats` rounds in which the variants alternate in one process.
Next to each: the bytes of reading every input once and writing every output once (for d the scratch image too, 4 bytes per
pixel each way) and bytes / time -- an ACCOUNTING, not a share of a measured peak.  The host time of the numpy restatement
(tests/photometric_ref.py) on one sample's 8 frames under d's program is printed for scale only.

    python tools/measure_train_photometric.py
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import photometric_ref as R  # noqa: E402
from thinktwice_amd import build, calib, photometric as P, synth  # noqa: E402
from thinktwice_amd.preprocess import IdaSampler, TrainImagePipeline  # noqa: E402


def main(B, repeats):
    T, N, H, W = 2, 4, calib.IMG_H, calib.IMG_W
    pipe = TrainImagePipeline(calib.IDA_AUG_CONF)
    fh, fw = pipe.final_dim
    NI = B * T * N
    raw = torch.from_numpy(np.stack([synth.raw_camera_frames(100 + b) for b in range(B)])).cuda()
    params = IdaSampler(calib.IDA_AUG_CONF, 7).sample(B, N)
    progs = {"b": [P.Program([], fh, fw) for _ in range(B)],
             "c": P.PhotometricSampler(B, seed=1).programs(B, fh, fw, iteration=0),
             "d": P.PhotometricSampler(B, seed=1).programs(B, fh, fw, iteration=1500000)}
    for k in "cd":
        print(f"  programs of {k}: {[repr(p) for p in progs[k]]}")
    assert all(p.blur_index >= 0 for p in progs["d"])
    fns = {"a": lambda: pipe(raw, params=params), "a'": lambda: pipe(raw, params=params)}
    for k in "bcd":
        fns[k] = lambda k=k: pipe(raw, params=params, augment=progs[k])
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
    base = raw.numel() + 2 * 4 * H * W + 4 * NI * 3 * fh * fw
    prog_bytes = B * ctypes.sizeof(P.AugProgram)
    blurred = {k: sum(p.blur_index >= 0 for p in v) * T * N for k, v in progs.items()}
    print(f"B = {B}: {NI} frames {H} x {W} -> {fh} x {fw}, NCHW f32; device events, {repeats} rounds after 3 warm-up rounds")
    for k in fns:
        nbytes = base if k.startswith("a") else base + prog_bytes + 2 * 4 * blurred[k] * fh * fw
        med = statistics.median(ms[k])
        print(f"  {k:2s} median {med:.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})   {nbytes / 1e6:.1f} MB read / written once "
              f"-> {nbytes / med / 1e6:.1f} GB/s by that accounting" + (f"   ({blurred[k]} frames through the blur)" if k in "bcd" else ""))
    ma, mb = statistics.median(ms["a"]), statistics.median(ms["a'"])
    print(f"  A/A: a' - a = {mb - ma:+.3f} ms ({(mb - ma) / ma * 100:+.2f} %)")
    for k in "bcd":
        print(f"  {k} - a = {statistics.median(ms[k]) - ma:+.3f} ms ({(statistics.median(ms[k]) - ma) / ma * 100:+.2f} %)")
    out = pipe(raw[:1].contiguous(), params=params[:1], augment=[P.Program([], fh, fw)])["img"].cpu().numpy().astype(np.float64)
    mean = np.asarray(calib.IMAGENET_MEAN).reshape(1, 1, 1, 3, 1, 1)
    std = np.asarray(calib.IMAGENET_STD).reshape(1, 1, 1, 3, 1, 1)
    u8 = np.ascontiguousarray(np.rint((out * std + mean) * 255).astype(np.uint8).reshape(1, T * N, 3, fh, fw).transpose(0, 1, 3, 4, 2))
    t0 = time.perf_counter()
    ref = R.apply_batch(u8, progs["d"][:1])
    dt = time.perf_counter() - t0
    got = P.apply_u8(torch.from_numpy(u8).cuda(), progs["d"][:1]).cpu().numpy()
    print(f"  numpy restatement of d's program 0 on the {T * N} frames of one sample: {dt:.2f} s (host clock, one pass); "
          f"{int((got != ref).sum())} bytes differ from the device")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured on the host")
    print("build", build.source_fingerprint(), "device", torch.cuda.get_device_name(0))
    main(a.batch, a.repeats)
