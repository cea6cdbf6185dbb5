"""Numbers behind profiles/png_encode.txt (one MI355X): png_encode.PngEncoder on the agent's four 900 x 1600 x 3 frames and on
the 64 + 32 + 32 images of a B = 8 batch (camera frames, depth ramps, tag maps: the image kinds of bench_png.py), next to what
it replaces on the host (PIL's save at its default level and at compress_level=1, png.segment_png), with the file sizes, the
decode time of the device-written files through png.PngDecoder, the host time of FrameRecorder.submit and the cost of a
recording AgentTick.

    python -m thinktwice_amd.bench_png_encode [--batch 8] [--repeats 5] [--ticks 40] [--out profiles/png_encode.txt]

Device times are event pairs around the call, interleaved, median of `repeats`; every comparison has its A/A twin (the same
call measured twice in the same interleaving) next to it.  Nothing here is a pass criterion."""
import argparse
import io
import statistics
import sys
import time

import numpy as np

from . import build, synth
from .bench_png import H, N, W, _depth_ramp, _events

TICK_MS = 15.5                                                     # AgentTick at the full size (profiles/r06_tick_last_tick.txt)


def _med(v):
    return statistics.median(v)


def _host_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return _med(out)


def _pil_save(a, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="PNG", **kw)
    return buf.getvalue()


def _phases(enc, tensors, phases):
    """The encoder's own call with the launches cut after `phases` (tt_png_encode_u8_phases), on its buffers."""
    import torch
    from .ops import check, lib, ptr
    table, views, pixel_bytes, files_bytes = enc._table_of(tensors)
    table_dev = torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).to(enc.device)
    need = int(lib().tt_png_encode_workspace_bytes(table, len(table)))
    pixels, work, files = enc._pixels, enc._work, enc._files
    assert pixels.numel() >= pixel_bytes and work.numel() >= need and files.numel() >= files_bytes

    def run():
        check(lib().tt_png_encode_u8_phases(ptr(pixels), pixel_bytes, table, ptr(table_dev), len(table), ptr(work), work.numel(),
                                            ptr(files), files_bytes, ptr(files), phases, torch.cuda.current_stream().cuda_stream),
              "tt_png_encode_u8_phases")
    run.keep = (table, table_dev)
    return run


def _sizes(emit, what, arrays, files, repeats):
    from . import png
    a = arrays[0]
    pil6, pil1 = _pil_save(a), _pil_save(a, compress_level=1)
    seg6 = png.segment_png(pil6, 16, 6)
    seg1 = png.segment_png(pil6, 16, 1)
    t6, t1 = _host_ms(lambda: _pil_save(a), repeats), _host_ms(lambda: _pil_save(a, compress_level=1), repeats)
    ts = _host_ms(lambda: png.segment_png(pil6, 16, 6), repeats)
    emit(f"  {what}: device file {len(files[0])} bytes; PIL default {len(pil6)} ({len(files[0]) / len(pil6):.3f} x), PIL compress_level=1 "
         f"{len(pil1)} ({len(files[0]) / len(pil1):.3f} x), segment_png level 6 {len(seg6)} ({len(files[0]) / len(seg6):.3f} x), level 1 "
         f"{len(seg1)} ({len(files[0]) / len(seg1):.3f} x)")
    emit(f"    host, one thread, one image: PIL save default {t6:.1f} ms, compress_level=1 {t1:.1f} ms; segment_png(level 6) of the "
         f"written file {ts:.1f} ms")
    return pil6


def main(B, repeats, ticks, emit):
    import torch
    from . import png, png_encode
    emit(f"build {build.source_fingerprint()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    _, tags, rgb = synth.raw_label_bytes(200, N, H, W)
    frames = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in rgb]
    enc = png_encode.PngEncoder()
    files = enc.encode(frames)
    dec = png.PngDecoder(segments="require", verify=True)
    assert torch.equal(dec.decode(files).cpu(), torch.from_numpy(np.stack(rgb)))
    emit(f"\nthe agent's four {H} x {W} x 3 frames, rows_per_segment 16, filter adaptive ({sum(len(f) for f in files)} file bytes)")
    runs = {p: _phases(enc, frames, p) for p in (1, 2, 3)}
    ms = _events({"encode": lambda: enc.encode(frames), "encode_aa": lambda: enc.encode(frames), "call": runs[3], "call_aa": runs[3],
                  "filter": runs[1], "filter + deflate": runs[2]}, repeats)
    m = {k: _med(v) for k, v in ms.items()}
    emit(f"  PngEncoder.encode (pixel staging, the call, the copy back, the host's bytes): {m['encode']:.2f} ms (A/A {m['encode_aa']:.2f})")
    emit(f"  tt_png_encode_u8 alone: {m['call']:.2f} ms (A/A {m['call_aa']:.2f}); filter pass {m['filter']:.2f} ms, deflate launch "
         f"{m['filter + deflate'] - m['filter']:.2f} ms, layout + compaction + checksums {m['call'] - m['filter + deflate']:.2f} ms")
    emit(f"  against the {TICK_MS} ms tick: the call is {m['call'] / TICK_MS:.2f} ticks of device time, on the tick's stream")
    pil = _sizes(emit, "camera frame", rgb, files, repeats)

    emit(f"\nB = {B}: {B * 2 * N} camera frames, {B * N} depth ramps, {B * N} tag maps in ONE call")
    cams, ramps, segs = [], [], []
    for b in range(B):
        _, t, key = synth.raw_label_bytes(200 + b, N, H, W)
        _, _, prev = synth.raw_label_bytes(300 + b, N, H, W)
        cams += list(prev) + list(key)
        ramps += [_depth_ramp(4 * b + n) for n in range(N)]
        segs += list(t)
    arrays = cams + ramps + segs
    batch = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    out = enc.encode(batch)
    runs = {p: _phases(enc, batch, p) for p in (1, 2, 3)}
    ms = _events({"encode": lambda: enc.encode(batch), "encode_aa": lambda: enc.encode(batch), "call": runs[3], "call_aa": runs[3],
                  "filter": runs[1], "filter + deflate": runs[2]}, repeats)
    m = {k: _med(v) for k, v in ms.items()}
    emit(f"  PngEncoder.encode: {m['encode']:.1f} ms (A/A {m['encode_aa']:.1f}); tt_png_encode_u8 alone {m['call']:.1f} ms (A/A "
         f"{m['call_aa']:.1f}): filter {m['filter']:.1f}, deflate {m['filter + deflate'] - m['filter']:.1f}, the rest "
         f"{m['call'] - m['filter + deflate']:.1f}")
    n_c, n_r = len(cams), len(ramps)
    ramp_pil = _sizes(emit, "depth ramp", ramps, out[n_c:], repeats)
    tag_pil = _sizes(emit, "tag map", segs, out[n_c + n_r:], repeats)
    # born segmented: the device-written files against the same images written by PIL, through the decoder
    plain = png.PngDecoder(segments="ignore")
    auto = png.PngDecoder(segments="auto")
    pil_cams = [_pil_save(a) for a in cams[:8]]
    ms = _events({"device-written": lambda: auto.decode(out[:8]), "device-written_aa": lambda: auto.decode(out[:8]),
                  "PIL-written": lambda: plain.decode(pil_cams)}, repeats)
    m = {k: _med(v) for k, v in ms.items()}
    emit(f"  PngDecoder.decode of 8 camera frames: device-written (segmented, no transcode) {m['device-written']:.2f} ms (A/A "
         f"{m['device-written_aa']:.2f}), PIL-written (one wave per file) {m['PIL-written']:.2f} ms")

    emit("\nFrameRecorder.submit on the caller's thread (four frames + two small files), against the PIL save of ONE frame")
    import tempfile
    with tempfile.TemporaryDirectory() as root:
        rec = png_encode.FrameRecorder(root, encoder=enc, max_pending=4)
        names = {f"cam{i}/0000.png": f for i, f in enumerate(frames)}
        rec.submit(names, {"meta/0000.json": b"{}"})
        torch.cuda.synchronize()
        t = []
        for k in range(max(repeats, 5)):
            t0 = time.perf_counter()
            rec.submit(names, {"meta/0000.json": b"{}"})
            t.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
            time.sleep(0.05)                                        # the writer thread drains: the next submit finds a free slot
        rec.close()
        emit(f"  submit: {_med(t):.2f} ms host time (min {min(t):.2f}, max {max(t):.2f}; {rec.stalls} stalls); PIL save of one frame "
             f"{_host_ms(lambda: _pil_save(rgb[0]), 3):.1f} ms")

        if ticks > 0:
            from . import model as tm, params
            from .agent_tick import AgentTick
            mdl, cfg = tm.build_thinktwice(dtype="f32x3")
            mdl.load_state_dict(params.init_params(cfg, seed=0))
            rec = png_encode.FrameRecorder(root, encoder=enc, max_pending=4)
            pair = {"recorder=None": AgentTick(mdl, lag=1, queue_len=2), "record_every=10": AgentTick(mdl, lag=1, queue_len=2, recorder=rec)}
            rng = np.random.default_rng(0)
            raw = torch.from_numpy(np.stack(rgb)).cuda()
            half = np.concatenate([rng.uniform(-8, 30, (10000, 1)), rng.uniform(-19, 19, (10000, 1)), rng.uniform(-4.5, 0.5, (10000, 1)),
                                   rng.uniform(0, 1, (10000, 1))], 1).astype(np.float32)
            args = (raw, half, np.array([12.0, -3.0]), 0.4, 3.0, np.array([21.0, 11.0]), 2)
            wall = {k: [] for k in pair}
            for i in range(ticks + 4):
                for k, tick in pair.items():                        # alternating, in one process
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tick.run_step(*args)
                    torch.cuda.synchronize()
                    if i >= 4:
                        wall[k].append((1e3 * (time.perf_counter() - t0), tick.step % 10 == 0))
            rec.close()
            base = _med([t for t, _ in wall["recorder=None"]])
            quiet = _med([t for t, r in wall["record_every=10"] if not r])
            loud = [t for t, r in wall["record_every=10"] if r]
            emit(f"\nAgentTick.run_step, {ticks} ticks each, alternating (wall, synchronised after every tick): recorder=None {base:.2f} ms; "
                 f"with a recorder {quiet:.2f} ms on the nine ticks that do not record (A/A of the same code), "
                 f"{_med(loud):.2f} ms on the recording tick ({len(loud)} of them; it waits here for the encode, which a tick that "
                 f"does not synchronise leaves on the stream); {rec.stalls} stalls")
    del pil, ramp_pil, tag_pil
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    rc = main(a.batch, a.repeats, a.ticks, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(rc)
