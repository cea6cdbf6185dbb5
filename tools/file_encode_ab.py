#!/usr/bin/env python
"""Per-phase device time of the two device file encoders under two builds of the library, interleaved in one process: the check
of a refactor after which tools/isa_compare.py reports a kernel of png_encode.hip or jpeg_encode.hip as different.

    python tools/file_encode_ab.py PARENT_LIB BRANCH_LIB [--repeats 15] [-o profiles/NAME.txt]

Workload: the agent's four 900 x 1600 x 3 camera frames, as in bench_png_encode / bench_jpeg_encode, on one encoder's buffers.  The
launches are cut by tt_png_encode_u8_phases / tt_jpeg_encode_u8_phases (1: the first pass; 2: and the coder; 3: the whole call).
Every phase is timed as parent, parent again (the A/A twin) and branch, in that interleaving, one event pair per call.  Per phase
the tool prints the three medians and the A/A spread, which is the distance between the parent's median and its twin's, as the
benches print it, and says whether the branch's median is at most that far from the parent's.  A phase whose kernels are the same
text in both builds shows what this measure does on equal code.  The benches themselves load one library per process
(TT_LIB_PATH); two in one process, which the interleaving needs, are loaded here.  Exit status 0: every phase inside, equal bytes."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def phase_call(so, fmt, enc, tensors, phases):
    """tt_<fmt>_encode_u8_phases of the library `so` on the encoder's own buffers."""
    import torch
    from thinktwice_amd.ops import ptr
    table, _, pixel_bytes, files_bytes = enc._table_of(tensors)
    table_dev = torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).to(enc.device)
    file_sizes = torch.zeros(len(table), dtype=torch.int64, device=enc.device)
    fn, pixels, work, files = getattr(so, f"tt_{fmt}_encode_u8_phases"), enc._pixels, enc._work, enc._files

    def run():
        rc = fn(ptr(pixels), pixel_bytes, table, ptr(table_dev), len(table), ptr(work), work.numel(), ptr(files), files_bytes,
                ptr(file_sizes), phases, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (fmt, phases, rc)
    run.keep = (table, table_dev)
    run.written = lambda: (files[:files_bytes].clone(), file_sizes.clone())
    return run


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("-o", "--output", help="also append the report to this file")
    a = ap.parse_args()
    import torch
    from thinktwice_amd import _lib, jpeg_encode, png_encode, synth
    from thinktwice_amd.bench_png import H, N, W, _events
    libs = {"parent": _lib.load(os.path.abspath(a.parent)), "branch": _lib.load(os.path.abspath(a.branch))}
    _, _, rgb = synth.raw_label_bytes(200, N, H, W)
    frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in rgb]
    out = [f"{torch.cuda.get_device_name(0)}; the agent's four {H} x {W} x 3 frames; {a.repeats} repeats, interleaved parent / parent / branch;",
           "ms: parent median, its A/A twin's median, branch median, |twin - parent| (the A/A spread), |branch - parent|"]
    all_inside = True
    for fmt, enc, names in (("png", png_encode.PngEncoder(), ("filter", "filter + deflate", "whole call")),
                            ("jpeg", jpeg_encode.JpegEncoder(quality=90, subsampling="420"), ("transform", "transform + entropy", "whole call"))):
        enc.encode(frames)                                              # (sizes the buffers, stages the pixels)
        fns = {}
        for p in (1, 2, 3):
            fns[p, "parent"] = phase_call(libs["parent"], fmt, enc, frames, p)
            fns[p, "parent_aa"] = fns[p, "parent"]
            fns[p, "branch"] = phase_call(libs["branch"], fmt, enc, frames, p)
        ms = _events(fns, a.repeats)
        for p, name in zip((1, 2, 3), names):
            pa, aa, br = (statistics.median(ms[p, k]) for k in ("parent", "parent_aa", "branch"))
            spread, off = abs(aa - pa), abs(br - pa)
            inside = off <= spread
            all_inside = all_inside and inside
            out.append(f"  tt_{fmt}_encode_u8_phases {p} ({name}): {pa:.4f}  {aa:.4f}  {br:.4f}  {spread:.4f}  {off:.4f}  "
                       f"branch {'inside' if inside else 'OUTSIDE'} the A/A spread")
        written = []
        for k in ("parent", "branch"):                                  # (zeroed first: a slot is written up to its file's size)
            enc._files.zero_()
            fns[3, k]()
            written.append(fns[3, k].written())
        same = all(torch.equal(x, y) for x, y in zip(*written))
        all_inside = all_inside and same
        out.append(f"  tt_{fmt}_encode_u8_phases 3: the file buffer and the file sizes of the two builds are {'equal' if same else 'DIFFERENT'}")
    out.append("RESULT: " + ("every phase inside the parent's A/A spread, equal bytes" if all_inside else
                             "a phase OUTSIDE the parent's A/A spread, or different bytes"))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if a.output:
        open(a.output, "a").write(text)
    return 0 if all_inside else 1


if __name__ == "__main__":
    sys.exit(main())
