"""Segment a dataset's PNG files once, on the host, so that png.PngDecoder can give every segment a wave of its own:

    python -m thinktwice_amd.png_segment SRC DST [--rows R] [--level L] [--workers N]

mirrors the directory tree SRC into DST: every `*.png` goes through png.segment_png (the same pixels, filter bytes and
validity; a full flush after every R rows and the `ttSG` index chunk), every other file is copied as it is.  A file that
png.parse_png refuses (a palette file, 16 bits, interlaced) is copied unchanged and counted.  SRC may also be one file, DST
then names the file to write.  Needs no GPU and does not load the HIP library's kernels."""
import argparse
import concurrent.futures
import os
import shutil
import sys

DEFAULT_ROWS = 16
MAX_WORKERS = 16


def _jobs(src, dst):
    if os.path.isfile(src):
        return [(src, dst)]
    out = []
    for root, _, names in os.walk(src):
        rel = os.path.relpath(root, src)
        for name in sorted(names):
            out.append((os.path.join(root, name), os.path.normpath(os.path.join(dst, rel, name))))
    return out


def _one(job):
    """-> (what happened, bytes read, bytes written)"""
    src, dst, rows, level = job
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    if not src.lower().endswith(".png"):
        shutil.copyfile(src, dst)
        return "copied", 0, 0
    from . import png
    data = open(src, "rb").read()
    try:
        out = png.segment_png(data, rows, level)
    except ValueError as e:
        shutil.copyfile(src, dst)
        return f"unchanged ({e})", 0, 0
    with open(dst, "wb") as f:
        f.write(out)
    return "segmented", len(data), len(out)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m thinktwice_amd.png_segment", description=__doc__.split("\n\n")[0])
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--rows", type=int, default=DEFAULT_ROWS, help="rows per segment (default %(default)s)")
    ap.add_argument("--level", type=int, default=6, help="zlib level (default %(default)s)")
    ap.add_argument("--workers", type=int, default=None, help=f"processes (default: one per file, at most {MAX_WORKERS})")
    a = ap.parse_args(argv)
    if a.rows < 1 or not -1 <= a.level <= 9:
        ap.error("--rows must be at least 1 and --level one of -1..9")
    if not os.path.exists(a.src):
        ap.error(f"{a.src} does not exist")
    if os.path.isdir(a.src) and os.path.abspath(a.dst).startswith(os.path.abspath(a.src) + os.sep):
        ap.error("DST lies inside SRC")
    jobs = [(s, d, a.rows, a.level) for s, d in _jobs(a.src, a.dst)]
    workers = max(1, min(a.workers if a.workers is not None else MAX_WORKERS, len(jobs)))
    if workers == 1:
        results = [_one(j) for j in jobs]
    else:
        with concurrent.futures.ProcessPoolExecutor(workers) as pool:
            results = list(pool.map(_one, jobs, chunksize=4))
    done = [r for r in results if r[0] == "segmented"]
    for (src, *_), r in zip(jobs, results):
        if r[0].startswith("unchanged"):
            print(f"{src}: {r[0]}", file=sys.stderr)
    before, after = sum(r[1] for r in done), sum(r[2] for r in done)
    print(f"{len(done)} files segmented at {a.rows} rows per segment ({before} -> {after} bytes"
          + (f", {after / before:.3f} x" if before else "") + f"), {sum(r[0] == 'copied' for r in results)} other files copied, "
          f"{sum(r[0].startswith('unchanged') for r in results)} PNG files left unchanged")
    return 0


if __name__ == "__main__":
    sys.exit(main())
