"""Numbers behind profiles/jpeg_encode.txt (one MI355X): jpeg_encode.JpegEncoder on the agent's four 900 x 1600 x 3 camera frames
and on a canvas of the debug renderer's default size (936 x 3584 x 3), beside png_encode.PngEncoder on the same tensors in the
same run and PIL's save(quality=...) on the host: device time per phase, wall time on the caller's thread, file sizes.  The
claim it establishes or refutes: a recorded tick with `render` no longer pays the PNG encoding of the canvas.

    python -m thinktwice_amd.bench_jpeg_encode [--repeats 7] [--quality 90] [--out profiles/jpeg_encode.txt]

Device times are event pairs around the call, interleaved, median of `repeats`; every comparison has its A/A twin (the same
call measured twice in the same interleaving) next to it.  The canvas is a stand-in with the renderer's proportions: camera
crops in the upper rows, flat panels with one-pixel glyph edges below.  Nothing here is a pass criterion."""
import argparse
import io
import sys
import time

import numpy as np

from . import build, synth
from .bench_png import H, N, W, _events
from .bench_png_encode import _host_ms, _med, _phases as _png_phases


def _pil_jpeg(a, quality, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=quality, subsampling={"444": 0, "420": 2}[subsampling], optimize=False)
    return buf.getvalue()


def _phases(enc, tensors, phases):
    """The encoder's own call with the launches cut after `phases` (tt_jpeg_encode_u8_phases), on its buffers."""
    import torch
    from .ops import check, lib, ptr
    table, views, pixel_bytes, files_bytes = enc._table_of(tensors)
    table_dev = torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).to(enc.device)
    need = int(lib().tt_jpeg_encode_workspace_bytes(table, len(table)))
    pixels, work, files = enc._pixels, enc._work, enc._files
    assert pixels.numel() >= pixel_bytes and work.numel() >= need and files.numel() >= files_bytes

    def run():
        check(lib().tt_jpeg_encode_u8_phases(ptr(pixels), pixel_bytes, table, ptr(table_dev), len(table), ptr(work), work.numel(),
                                             ptr(files), files_bytes, ptr(files), phases, torch.cuda.current_stream().cuda_stream),
              "tt_jpeg_encode_u8_phases")
    run.keep = (table, table_dev)
    return run


def debug_canvas(frames, height=936, width=3584):
    """uint8 [height, width, 3] with the debug frame's proportions: the four camera frames' crops across the upper 448 rows, a
    dark panel with flat rectangles and rows of 5 x 7 glyph-like bit patterns below."""
    rng = np.random.default_rng(7)
    out = np.full((height, width, 3), (24, 24, 32), dtype=np.uint8)
    for i, f in enumerate(frames):
        out[:448, 896 * i:896 * (i + 1)] = f[200:648, 300:1196]
    out[500:900, 100:900] = (40, 90, 200)
    out[520:880, 1800:2600] = (200, 40, 40)
    for y in range(470, height - 8, 10):
        for x in range(1000, 1700, 7):
            glyph = rng.integers(0, 2, (7, 5)).astype(bool)
            out[y:y + 7, x:x + 5][glyph] = (235, 235, 235)
    return out


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def _workload(emit, what, arrays, quality, subsampling, repeats):
    import torch
    from PIL import Image
    from . import jpeg_encode, png_encode
    tensors = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    jenc = jpeg_encode.JpegEncoder(quality=quality, subsampling=subsampling)
    penc = png_encode.PngEncoder()
    jfiles, pfiles = jenc.encode(tensors), penc.encode(tensors)
    jruns = {p: _phases(jenc, tensors, p) for p in (1, 2, 3)}
    pcall = _png_phases(penc, tensors, 3)
    ms = _events({"jpeg encode": lambda: jenc.encode(tensors), "jpeg encode_aa": lambda: jenc.encode(tensors),
                  "png encode": lambda: penc.encode(tensors), "jpeg call": jruns[3], "jpeg call_aa": jruns[3], "png call": pcall,
                  "png call_aa": pcall, "transform": jruns[1], "transform + entropy": jruns[2]}, repeats)
    m = {k: _med(v) for k, v in ms.items()}
    emit(f"\n{what}: quality {quality}, {subsampling}, restart_rows 1")
    emit(f"  tt_jpeg_encode_u8 alone: {m['jpeg call']:.3f} ms device (A/A {m['jpeg call_aa']:.3f}): transform {m['transform']:.3f}, entropy "
         f"{m['transform + entropy'] - m['transform']:.3f}, layout + compaction {m['jpeg call'] - m['transform + entropy']:.3f}")
    emit(f"  tt_png_encode_u8 alone, the same tensors, the same run: {m['png call']:.3f} ms device (A/A {m['png call_aa']:.3f}); "
         f"JPEG / PNG = {m['jpeg call'] / m['png call']:.3f}")
    emit(f"  encode() (pixel staging, the call, the copy of the slots, the host's bytes), event pair: JPEG {m['jpeg encode']:.2f} ms "
         f"(A/A {m['jpeg encode_aa']:.2f}), PNG {m['png encode']:.2f} ms")

    def wall(enc):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pending = enc.encode_async(tensors)
        t1 = time.perf_counter()
        pending.result()
        return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t0)
    for name, enc in (("JPEG", jenc), ("PNG", penc)):
        w = [wall(enc) for _ in range(max(repeats, 5))]
        emit(f"  {name} wall on the caller's thread: encode_async returns after {_med([a for a, _ in w]):.2f} ms, result() is there after "
             f"{_med([b for _, b in w]):.2f} ms")
    a = arrays[0]
    pil = _pil_jpeg(a, quality, subsampling)
    t_pil = _host_ms(lambda: _pil_jpeg(a, quality, subsampling), max(3, repeats // 2))
    ours = np.asarray(Image.open(io.BytesIO(jfiles[0])))
    theirs = np.asarray(Image.open(io.BytesIO(pil)))
    emit(f"  files: JPEG {[len(f) for f in jfiles]} bytes, PNG {[len(f) for f in pfiles]} bytes (JPEG / PNG = "
         f"{sum(map(len, jfiles)) / sum(map(len, pfiles)):.4f}); PIL save(quality={quality}) of the first: {len(pil)} bytes, {t_pil:.1f} ms "
         f"on one host thread")
    emit(f"  first image, PSNR against the source: ours {_psnr(ours, a):.2f} dB, PIL's {_psnr(theirs, a):.2f} dB")
    return m


def main(repeats, quality, emit):
    import torch
    emit(f"build {build.source_fingerprint()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    _, _, rgb = synth.raw_label_bytes(200, N, H, W)
    rgb = [np.ascontiguousarray(a) for a in rgb]
    cams = _workload(emit, f"the agent's four {H} x {W} x 3 camera frames", rgb, quality, "420", repeats)
    canvas = debug_canvas(rgb)
    dbg = _workload(emit, f"one debug canvas {canvas.shape[0]} x {canvas.shape[1]} x 3", [canvas], quality, "420", repeats)
    emit(f"\nthe claim: a recorded tick with render pays the canvas's encoding. PNG {dbg['png call']:.2f} ms -> JPEG "
         f"{dbg['jpeg call']:.2f} ms of device time for the canvas; the four camera frames PNG {cams['png call']:.2f} ms -> JPEG "
         f"{cams['jpeg call']:.2f} ms")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    rc = main(a.repeats, a.quality, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(rc)
