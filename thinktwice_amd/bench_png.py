"""Numbers behind profiles/train_png_decode.txt (one MI355X): png.PngDecoder on one B = 8 batch of dataset-sized files (64 camera
frames, 32 depth maps, 32 segmentation maps of 900 x 1600), against PIL decoding the same files on the same box.

    python -m thinktwice_amd.bench_png [--batch 8] [--repeats 5] [--train-step-ms 750] [--out profiles/train_png_decode.txt]

The camera frames and the tags are synth.raw_label_bytes'; the depth maps are a smooth ramp in CARLA's 24-bit code, and once
more that function's all-random depth bytes (incompressible: the stored-block extreme).  The files are written by PIL when it
is importable, else by the test writer (tests/png_cases.py) at zlib level 6.  PIL's decode is timed first, on the host clock,
with 1 and with 16 processes, before this process touches the device (the pool forks).  Then device events around each call
after one warm-up round, the variants alternating in one process: the whole decode_sample_batch call (parse, pack, copy, two
launches, status read-back) twice (A/A), the host-to-device copy alone, the inflate launch alone (tt_png_decode_u8_phases) and
both launches; the unfilter is their difference.  --train-step-ms: the train_step time of `bench.py --full` at the parent
commit on the same machine, which the whole call is set against.

    python -m thinktwice_amd.bench_png --verify [--batch 8] [--repeats 5] [--out profiles/train_png_verify.txt]

--verify measures instead what PngDecoder(verify=...) adds (tt_png_decode_u8_verified: the Adler-32 of every stream and the
CRC-32 of every IDAT chunk, on the device): the whole decode_sample_batch call with verification off, off again (A/A), with
("adler32",) and with ("adler32", "crc32"), and the inflate launch alone, alternating in one process; then the checksum
kernels on their own (png.device_adler32 / device_crc32 over the same number of bytes).  The cost of verification is the
verify-on median minus the verify-off median, to be read against the A/A spread.  Without the switch the output is as before.

    python -m thinktwice_amd.bench_png --segment-rows 8,16,32,64 [--batch 8] [--repeats 5] [--train-step-ms 735]
                                       [--out profiles/train_png_segmented.txt]

--segment-rows measures instead the segmented decode (png.segment_png, tt_png_decode_u8_segmented: one wave per segment) for
every R of the list: the batch is segmented on the host first (16 processes, not counted: it is done once per dataset), the
file-size ratio is reported per image kind, and then, alternating in one process, the whole decode_sample_batch call on the
unsegmented files twice (A/A; that path is the parent's) and on the files of every R, twice each, and the inflate launch
alone for each (tt_png_decode_u8_phases, tt_png_decode_u8_segmented_phases)."""
import argparse
import io
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np

from . import build, synth

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
N, T, H, W = 4, 2, 900, 1600
_FILES = []                                                        # what the forked PIL workers decode


def _depth_ramp(seed):
    yy, xx = np.mgrid[0:H, 0:W]
    a, b = 5 + seed % 7, 3 + seed % 5
    code = ((yy * a + xx * b) * 16777215 // (H * a + W * b)).astype(np.uint32)
    return np.stack([code & 255, (code >> 8) & 255, code >> 16], axis=-1).astype(np.uint8)


def _writer():
    try:
        from PIL import Image

        def write(a):
            buf = io.BytesIO()
            Image.fromarray(a).save(buf, format="PNG")
            return buf.getvalue()
        import PIL
        return write, f"PIL {PIL.__version__} (Image.fromarray(a).save)"
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import png_cases
        return (lambda a: png_cases.write_png(a, [y % 5 for y in range(a.shape[0])], compressor="level6"),
                "tests/png_cases.py at zlib level 6, filter types cycling 0..4 (PIL is not installed)")


def make_batch(B, write):
    """(rgb_files [B][T][N], depth_files [B][N], random_depth_files [B][N], seg_files [B][N], the source arrays alike)."""
    files, arrays = ([], [], [], []), ([], [], [], [])
    for b in range(B):
        depth_rand, tags, key = synth.raw_label_bytes(200 + b, N, H, W)
        _, _, prev = synth.raw_label_bytes(300 + b, N, H, W)
        ramps = [_depth_ramp(4 * b + n) for n in range(N)]
        for k, per_sample in enumerate(([list(prev), list(key)], ramps, list(depth_rand), list(tags))):
            arrays[k].append(per_sample)
            files[k].append([[write(a) for a in t] for t in per_sample] if k == 0 else [write(a) for a in per_sample])
    return files, arrays


def _pil_decode(i):
    from PIL import Image
    return int(np.array(Image.open(io.BytesIO(_FILES[i]))).shape[0])


def _pil_times(flat):
    try:
        import PIL  # noqa: F401
    except ImportError:
        return None
    _FILES[:] = flat
    t0 = time.perf_counter()
    for i in range(len(flat)):
        _pil_decode(i)
    one = time.perf_counter() - t0
    with multiprocessing.get_context("fork").Pool(16) as pool:
        pool.map(_pil_decode, range(16))                           # the workers are up
        t0 = time.perf_counter()
        pool.map(_pil_decode, range(len(flat)), chunksize=1)
        many = time.perf_counter() - t0
    return one, many


def _events(fns, repeats):
    import torch
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


def main(B, repeats, train_step_ms, emit):
    write, writer = _writer()
    t0 = time.perf_counter()
    (rgb_f, ramp_f, rand_f, seg_f), (rgb_a, ramp_a, rand_a, seg_a) = make_batch(B, write)
    flat = [f for s in rgb_f for t in s for f in t] + [f for s in ramp_f for f in s] + [f for s in seg_f for f in s]
    emit(f"B = {B}: {len(flat)} files of {H} x {W} ({B * T * N} camera frames, {B * N} depth maps, {B * N} segmentation maps) written "
         f"by {writer}; made in {time.perf_counter() - t0:.0f} s")
    sizes = [sum(len(f) for s in rgb_f for t in s for f in t)] + [sum(len(f) for s in v for f in s) for v in (ramp_f, rand_f, seg_f)]
    decoded = B * (T + 1) * N * H * W * 3 + B * N * H * W
    emit(f"  compressed bytes: camera frames {sizes[0]}, depth ramps {sizes[1]} (all-random depth instead: {sizes[2]}), tags {sizes[3]}; "
         f"decoded bytes {decoded}")
    pil = _pil_times(flat)
    if pil:
        emit(f"  PIL decoding the same {len(flat)} files on this box, host clock, one pass: 1 process {pil[0]:.2f} s "
             f"({pil[0] / len(flat) * 1e3:.0f} ms per file), 16 processes {pil[1]:.2f} s")

    import torch
    from . import png
    from .ops import check, cur_stream, lib, ptr
    emit(f"build {build.source_fingerprint()} device {torch.cuda.get_device_name(0)}")
    dec = png.PngDecoder()
    for what, depth_f, depth_a in (("depth ramps", ramp_f, ramp_a), ("all-random depth bytes", rand_f, rand_a)):
        raw, depth, seg = dec.decode_sample_batch(rgb_f, depth_f, seg_f)
        bad = int((raw.cpu() != torch.from_numpy(np.array(rgb_a))).sum()) + int((depth.cpu() != torch.from_numpy(np.array(depth_a))).sum())
        bad += int((seg.cpu() != torch.from_numpy(np.array(seg_a))).sum())
        emit(f"  [{what}] device against the source arrays: {bad} of {decoded} bytes differ")
        del raw, depth, seg
        infos = [png.parse_png(f) for f in [f for s in rgb_f for t in s for f in t] + [f for s in depth_f for f in s]
                 + [f for s in seg_f for f in s]]
        offsets, pos = [], 0
        for i in infos:
            offsets.append(pos)
            pos += i.width * i.height * i.channels
        out = torch.empty(pos, dtype=torch.uint8, device="cuda")
        table, total = dec._pack(infos, offsets)
        need = int(lib().tt_png_workspace_bytes(table, len(infos)))
        staged = dec._stage[:total].clone().pin_memory()             # this layout's own copies: the timed calls below repack dec's
        packed, work = staged.cuda(), dec._work
        status = torch.zeros(len(infos), dtype=torch.int32, device="cuda")
        stream = cur_stream(out.device)

        def launches(phases):
            check(lib().tt_png_decode_u8_phases(ptr(packed), total, table, ptr(packed), len(infos), ptr(work), work.numel(), ptr(out),
                                                pos, ptr(status), phases, stream), "tt_png_decode_u8_phases")

        fns = {"call": lambda: dec.decode_sample_batch(rgb_f, depth_f, seg_f), "call'": lambda: dec.decode_sample_batch(rgb_f, depth_f, seg_f),
               "h2d": lambda: packed.copy_(staged, non_blocking=True),
               "inflate": lambda: launches(1), "both": lambda: launches(2)}
        ms = _events(fns, repeats)
        med = {k: statistics.median(v) for k, v in ms.items()}
        emit(f"  [{what}] device events around each call, {repeats} rounds after 1 warm-up round, the variants alternating in one process")
        for k, label in (("call", "decode_sample_batch (parse, pack, copy, 2 launches, status read-back)"), ("call'", "the same again (A/A)"),
                         ("h2d", f"the pinned host-to-device copy alone ({total} bytes)"), ("inflate", "inflate launch alone"),
                         ("both", "inflate + unfilter launches")):
            emit(f"    {label:74s} median {med[k]:9.2f} ms (min {min(ms[k]):.2f}, max {max(ms[k]):.2f})")
        spread = med["call'"] - med["call"]
        emit(f"    unfilter by difference: {med['both'] - med['inflate']:+.2f} ms; A/A spread {spread:+.2f} ms; workspace {need} bytes")
        emit(f"    inflate rate: {decoded / med['inflate'] / 1e6:.2f} GB/s of scanlines over {len(infos)} workgroups "
             f"({decoded / len(infos) / med['inflate'] / 1e3:.1f} MB/s per stream)")
        emit(f"    whole call / a {train_step_ms:.0f} ms train_step at B = {B}: {med['call'] / train_step_ms * 100:.1f} %")
        if pil:
            emit(f"    PIL on one core / the whole call: {pil[0] * 1e3 / med['call']:.1f} x; host cores freed at one batch per train_step: "
                 f"{pil[0] * 1e3 / train_step_ms:.1f}")


def main_verify(B, repeats, emit):
    import torch
    from . import png
    from .ops import check, cur_stream, lib, ptr
    write, writer = _writer()
    t0 = time.perf_counter()
    (rgb_f, ramp_f, _, seg_f), (rgb_a, ramp_a, _, seg_a) = make_batch(B, write)
    flat = [f for s in rgb_f for t in s for f in t] + [f for s in ramp_f for f in s] + [f for s in seg_f for f in s]
    decoded = B * (T + 1) * N * H * W * 3 + B * N * H * W
    chunks = sum(len(png._walk(f, False)[3]) for f in flat)
    emit(f"B = {B}: {len(flat)} files of {H} x {W} written by {writer}; made in {time.perf_counter() - t0:.0f} s; {sum(map(len, flat))} file "
         f"bytes in {chunks} IDAT chunks, {decoded} decoded bytes")
    emit(f"build {build.source_fingerprint()} device {torch.cuda.get_device_name(0)}")
    decoders = {"off": png.PngDecoder(), "off'": png.PngDecoder(), "adler32": png.PngDecoder(verify=("adler32",)),
                "adler32 + crc32": png.PngDecoder(verify=True)}
    for name, dec in decoders.items():
        raw, depth, seg = dec.decode_sample_batch(rgb_f, ramp_f, seg_f)
        bad = int((raw.cpu() != torch.from_numpy(np.array(rgb_a))).sum()) + int((depth.cpu() != torch.from_numpy(np.array(ramp_a))).sum())
        bad += int((seg.cpu() != torch.from_numpy(np.array(seg_a))).sum())
        emit(f"  [verify {name}] every status TT_PNG_OK; device against the source arrays: {bad} of {decoded} bytes differ")
        del raw, depth, seg
    dec = decoders["off"]
    infos = [png.parse_png(f) for f in flat]
    offsets, pos = [], 0
    for i in infos:
        offsets.append(pos)
        pos += i.width * i.height * i.channels
    out = torch.empty(pos, dtype=torch.uint8, device="cuda")
    table, total = dec._pack(infos, offsets)
    staged = dec._stage[:total].clone()
    packed, work = staged.cuda(), dec._work
    status = torch.zeros(len(infos), dtype=torch.int32, device="cuda")
    stream = cur_stream(out.device)
    lines, at = [], 0                                                  # every image's scanlines in the workspace
    for i in infos:
        lines.append((at, i.height * (1 + i.width * i.channels)))
        at += (lines[-1][1] + 255) // 256 * 256
    bodies = [(int(im.stream_offset), int(im.stream_bytes)) for im in table]

    def inflate():
        check(lib().tt_png_decode_u8_phases(ptr(packed), total, table, ptr(packed), len(infos), ptr(work), work.numel(), ptr(out), pos,
                                            ptr(status), 1, stream), "tt_png_decode_u8_phases")

    fns = {k: (lambda d=d: d.decode_sample_batch(rgb_f, ramp_f, seg_f)) for k, d in decoders.items()}
    fns["inflate"] = inflate
    fns["adler kernels"] = lambda: png.device_adler32(work, lines)
    fns["crc kernels"] = lambda: png.device_crc32(packed, bodies)
    ms = _events(fns, repeats)
    med = {k: statistics.median(v) for k, v in ms.items()}
    emit(f"  device events around each call, {repeats} rounds after 1 warm-up round, the variants alternating in one process")
    labels = {"off": "decode_sample_batch, verify=()", "off'": "the same again (A/A)", "adler32": 'decode_sample_batch, verify=("adler32",)',
              "adler32 + crc32": 'decode_sample_batch, verify=("adler32", "crc32")', "inflate": "inflate launch alone (tt_png_decode_u8_phases)",
              "adler kernels": f"device_adler32 alone: {len(lines)} ranges, {sum(n for _, n in lines)} bytes (table upload + 3 launches)",
              "crc kernels": f"device_crc32 alone: {len(bodies)} ranges, {sum(n for _, n in bodies)} bytes (table upload + 3 launches)"}
    for k, label in labels.items():
        emit(f"    {label:88s} median {med[k]:9.2f} ms (min {min(ms[k]):.2f}, max {max(ms[k]):.2f})")
    spread = med["off'"] - med["off"]
    emit(f"    A/A spread {spread:+.2f} ms; adler32 - off {med['adler32'] - med['off']:+.2f} ms; "
         f"adler32 + crc32 - off {med['adler32 + crc32'] - med['off']:+.2f} ms; inflate launch {med['inflate']:.2f} ms")


def _segment_one(job):
    from . import png
    i, rows = job
    return png.segment_png(_FILES[i], rows)


def _nest_like(nest, flat):
    """`flat` (an iterator) poured into the shape of the nested lists `nest`."""
    return [_nest_like(x, flat) if isinstance(x, list) else next(flat) for x in nest]


def main_segments(B, repeats, rows_list, train_step_ms, emit):
    write, writer = _writer()
    t0 = time.perf_counter()
    (rgb_f, ramp_f, _, seg_f), (rgb_a, ramp_a, _, seg_a) = make_batch(B, write)
    kinds = (("camera frames", rgb_f), ("depth ramps", ramp_f), ("tags", seg_f))
    flat = [f for s in rgb_f for t in s for f in t] + [f for s in ramp_f for f in s] + [f for s in seg_f for f in s]
    n_rgb, n_dep = B * T * N, B * N
    decoded = B * (T + 1) * N * H * W * 3 + B * N * H * W
    emit(f"B = {B}: {len(flat)} files of {H} x {W} ({n_rgb} camera frames, {n_dep} depth maps, {n_dep} segmentation maps) written by "
         f"{writer}; made in {time.perf_counter() - t0:.0f} s; {sum(map(len, flat))} file bytes, {decoded} decoded bytes")
    _FILES[:] = flat
    nests = {}
    with multiprocessing.get_context("fork").Pool(16) as pool:       # before this process touches the device
        for rows in rows_list:
            t0 = time.perf_counter()
            out = pool.map(_segment_one, [(i, rows) for i in range(len(flat))], chunksize=1)
            took = time.perf_counter() - t0
            it = iter(out)
            nests[rows] = tuple(_nest_like(nest, it) for _, nest in kinds)
            sizes = [sum(len(f) for f in out[a:b]) for a, b in ((0, n_rgb), (n_rgb, n_rgb + n_dep), (n_rgb + n_dep, len(out)))]
            before = [sum(len(f) for f in flat[a:b]) for a, b in ((0, n_rgb), (n_rgb, n_rgb + n_dep), (n_rgb + n_dep, len(out)))]
            emit(f"  R = {rows:3d}: segmented at zlib level 6 by 16 host processes in {took:.1f} s (not counted below); "
                 f"{-(-H // rows)} segments per image, {len(flat) * -(-H // rows)} per batch; file bytes / unsegmented: "
                 + ", ".join(f"{k} {a / b:.3f}" for (k, _), a, b in zip(kinds, sizes, before)) + f", all {sum(sizes) / sum(before):.3f}")

    import torch
    from . import png
    from .ops import check, cur_stream, lib, ptr
    emit(f"build {build.source_fingerprint()} device {torch.cuda.get_device_name(0)}")
    want = [torch.from_numpy(np.array(a)) for a in (rgb_a, ramp_a, seg_a)]
    plain = png.PngDecoder()
    fns = {"plain": lambda: plain.decode_sample_batch(rgb_f, ramp_f, seg_f), "plain'": lambda: plain.decode_sample_batch(rgb_f, ramp_f, seg_f)}
    labels = {"plain": "unsegmented files: decode_sample_batch (parse, pack, copy, 2 launches, status read-back)",
              "plain'": "the same again (A/A)"}
    keep = []                                                          # the buffers of the launch-only variants

    def launch_only(files, label):
        dec = png.PngDecoder()
        infos = dec._parse(files)
        offsets, pos = [], 0
        for i in infos:
            offsets.append(pos)
            pos += i.width * i.height * i.channels
        out = torch.empty(pos, dtype=torch.uint8, device="cuda")
        table, total = dec._pack(infos, offsets)
        packed = dec._stage[:total].clone().cuda()
        segs, segs_at = dec._segs or (None, 0)
        need = int(lib().tt_png_segmented_workspace_bytes(table, len(infos), None, 0, 0, segs, len(segs) if segs else 0))
        work = torch.empty(need, dtype=torch.uint8, device="cuda")
        status = torch.zeros(len(infos), dtype=torch.int32, device="cuda")
        stream = cur_stream(out.device)
        keep.append((dec, table, segs, packed, work, out, status))

        def run():
            if segs:
                check(lib().tt_png_decode_u8_segmented_phases(ptr(packed), total, table, ptr(packed), len(infos), None, None, 0, 0, segs,
                                                              ptr(packed) + segs_at, len(segs), ptr(work), need, ptr(out), pos, ptr(status),
                                                              1, stream), "tt_png_decode_u8_segmented_phases")
            else:
                check(lib().tt_png_decode_u8_phases(ptr(packed), total, table, ptr(packed), len(infos), ptr(work), need, ptr(out), pos,
                                                    ptr(status), 1, stream), "tt_png_decode_u8_phases")
        fns[label] = run

    launch_only(flat, "plain inflate")
    labels["plain inflate"] = f"unsegmented files: inflate launch alone ({len(flat)} workgroups)"
    for rows in rows_list:
        r, d, s = nests[rows]
        dec = png.PngDecoder(segments="require")
        raw, depth, seg = dec.decode_sample_batch(r, d, s)
        bad = sum(int((got.cpu() != w).sum()) for got, w in zip((raw, depth, seg), want))
        emit(f"  [R = {rows}] every status TT_PNG_OK; device against the source arrays: {bad} of {decoded} bytes differ")
        del raw, depth, seg
        fns[f"R{rows}"] = lambda dec=dec, r=r, d=d, s=s: dec.decode_sample_batch(r, d, s)
        labels[f"R{rows}"] = f"R = {rows}: decode_sample_batch (parse, pack, copy, 4 launches, status read-back)"
        fns[f"R{rows}'"] = fns[f"R{rows}"]
        labels[f"R{rows}'"] = f"R = {rows}: the same again (A/A)"
        seg_flat = [f for x in r for t in x for f in t] + [f for x in d for f in x] + [f for x in s for f in x]
        launch_only(seg_flat, f"R{rows} inflate")
        labels[f"R{rows} inflate"] = (f"R = {rows}: inflate launch and the statuses' fold alone "
                                      f"({len(flat) * -(-H // rows)} + {len(flat)} workgroups)")
    ms = _events(fns, repeats)
    med = {k: statistics.median(v) for k, v in ms.items()}
    emit(f"  device events around each call, {repeats} rounds after 1 warm-up round, the variants alternating in one process")
    for k, label in labels.items():
        emit(f"    {label:100s} median {med[k]:9.2f} ms (min {min(ms[k]):.2f}, max {max(ms[k]):.2f})")
    spreads = [("unsegmented", med["plain'"] - med["plain"])] + [(f"R = {r}", med[f"R{r}'"] - med[f"R{r}"]) for r in rows_list]
    emit("    A/A spread: " + ", ".join(f"{k} {v:+.2f} ms" for k, v in spreads))
    for rows in rows_list:
        emit(f"    R = {rows:3d}: whole call {med[f'R{rows}']:8.2f} ms = {med[f'R{rows}'] / train_step_ms * 100:5.1f} % of a {train_step_ms:.0f} ms "
             f"train_step at B = {B}, {med['plain'] / med[f'R{rows}']:.1f} x the unsegmented call; inflate launch "
             f"{med[f'R{rows} inflate']:8.2f} ms, {med['plain inflate'] / med[f'R{rows} inflate']:.1f} x, "
             f"{decoded / med[f'R{rows} inflate'] / 1e6:.2f} GB/s of scanlines")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--train-step-ms", type=float, default=750.0)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--verify", action="store_true", help="measure what PngDecoder(verify=...) adds instead")
    ap.add_argument("--segment-rows", default=None, help="R[,R...]: measure the segmented decode at these rows per segment instead")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if a.segment_rows:
        main_segments(a.batch, a.repeats, [int(r) for r in a.segment_rows.split(",")], a.train_step_ms, emit)
    elif a.verify:
        main_verify(a.batch, a.repeats, emit)
    else:
        main(a.batch, a.repeats, a.train_step_ms, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
