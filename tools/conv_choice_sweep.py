"""Which kernel tt_conv2d_fwd picks, over a fixed list of layers that reaches every launch site of the dispatch and both sides of
every numeric threshold in it (csrc/conv_choose.cpp).

  --launch  (GPU) real buffers through ops.conv2d / ops.gather_conv; records the descriptor each call handed to the library and
            tt_conv_last_kernel() after it (or the error text of a refused layer).
  --plan    (no GPU) the same descriptors with dummy aligned addresses through tt_conv2d_plan.
  --query   (no GPU) only the QUERIES rows: layers ops.conv2d never asks the split-K query about (it asks for rows <= 4096 and
            K >= 2048) but tt_conv2d_splitk_slices answers for -- the far bounds of the bf16x3 split-K rule.  They are never launched;
            --launch and --plan carry them too, with the count the library under test gives.

Both print one JSON document (--out FILE writes it): {"cases": [{"name", "desc", "label", "query"?}]}.  `desc` holds every field of
tt_conv_desc that is not zero, pointers as 1; `query` is the tt_conv2d_splitk_slices answer where the caller asked (QUERIES rows have
no label under --launch / --query).  tests/conv_choice_cases.json is the --launch output of the commit before the dispatch moved into
one function (its QUERIES rows: that commit's --query, host only); tests/test_conv_choice.py replays it through tt_conv2d_plan.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

DT = {"f32": 0, "bf16": 1, "f16": 2}


def D(name, N, H, W, Cin, Cout, k=1, stride=1, pad=None, dt="f32", x3=False, h2=False, in_pair=False, out_pair=False, ws=False,
      cs=None, in_coff=0, in_cstride=None, out_hw=None, out2=False, ps2=False, res=0):
    """A dense layer: ops.conv2d's arguments.  k: int or (KH, KW); cs: channels of the input buffer (> Cin: a channel window at
    in_coff); ws: an explicit one-slice (atomic form) split-K workspace; res: residuals of the output's shape."""
    KH, KW = (k, k) if isinstance(k, int) else k
    return dict(kind="dense", name=name, N=N, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride,
                pad=(KH // 2 if KH == KW else 0) if pad is None else pad, dt=dt, x3=x3, h2=h2, in_pair=in_pair, out_pair=out_pair, ws=ws,
                cs=cs or Cin, in_coff=in_coff, in_cstride=in_cstride, out_hw=out_hw, out2=out2, ps2=ps2, res=res)


def S(name, M, Cin, Cout, stride=1, dt="f32", x3=False, plan=False):
    """A sparse 3x3x3 layer over the first M rows of a fully occupied 2 x 4 x 20 x 20 grid's rulebook (ops.gather_conv)."""
    return dict(kind="sparse", name=name, M=M, Cin=Cin, Cout=Cout, stride=stride, dt=dt, x3=x3, plan=plan)


GRID = (2, 4, 20, 20)        # 3200 rows in cell order

CASES = [
    # ---- "h2": half storage x f16 (hi, lo) weights.  64- / 128-wide, the pipe kernel from K = 1152 on Cout % 128 == 0; 31 taps at most
    D("h2 64-wide", 1, 1, 300, 64, 64, dt="f16", h2=True),
    D("h2 Cout=65", 1, 1, 300, 64, 65 + 7, dt="f16", h2=True),
    D("h2 128-wide", 1, 1, 300, 64, 128, dt="f16", h2=True),
    D("h2 K=1088", 1, 1, 300, 1088, 128, dt="f16", h2=True),
    D("h2 pipe K=1152", 1, 1, 300, 1152, 128, dt="f16", h2=True),
    D("h2 K=1152 Cout=192", 1, 1, 300, 1152, 192, dt="f16", h2=True),
    D("h2 pipe 3x3", 2, 24, 24, 128, 256, k=3, dt="f16", h2=True),
    D("h2 31 taps", 1, 40, 8, 64, 64, k=(31, 1), dt="f16", h2=True),
    D("h2 32 taps", 1, 40, 8, 64, 64, k=(32, 1), dt="f16", h2=True),
    D("h2 Cin=32", 1, 1, 300, 32, 64, dt="f16", h2=True),
    # ---- small (M <= 4096, <= 4096 tiles of 32 x 32) against the LDS-DMA kernels (M >= 2048)
    D("small M=300", 1, 1, 300, 64, 64),
    D("small 16-bit", 1, 1, 300, 64, 64, dt="bf16"),
    D("small x3 M=4096", 1, 64, 64, 64, 64, x3=True),
    D("x3 M=4097", 1, 1, 4097, 64, 64, x3=True),
    D("x3 M=2048 4160 tiles", 1, 1, 2048, 64, 2080, x3=True),
    D("x3 M=2047 4160 tiles", 1, 1, 2047, 64, 2080, x3=True),
    D("small M=2048 4096 tiles", 1, 1, 2048, 64, 2048, x3=True),
    D("small pixel shuffle", 1, 16, 16, 32, 64, ps2=True),
    D("out2 keeps a few-row layer off small", 1, 10, 30, 64, 64, x3=True, out2=True),
    # ---- bf16x3 tile width (cost model over 256 / 128 / 64), K < 1152: the compiler-scheduled tiles
    D("x3 Cout=64", 1, 64, 128, 32, 64, k=3, x3=True),
    D("x3 Cout=65", 1, 64, 128, 32, 68, k=3, x3=True),
    D("x3 Cout=128", 1, 64, 128, 32, 128, k=3, x3=True),
    D("x3 Cout=256 32 row tiles", 1, 64, 128, 32, 256, k=3, x3=True),
    D("x3 Cout=512 32 row tiles", 1, 64, 128, 32, 512, k=3, x3=True),
    D("x3 Cout=516", 1, 64, 128, 32, 516, k=3, x3=True),
    D("x3 Cout=640 wide, not a multiple of 256", 1, 128, 256, 64, 640, x3=True),
    D("x3 255 row tiles Cout=256", 1, 255, 256, 64, 256, x3=True),
    D("x3 256 row tiles Cout=256", 1, 256, 256, 64, 256, x3=True),
    D("x3 257 row tiles Cout=256", 1, 257, 256, 64, 256, x3=True),
    D("x3 128-wide: 200 row tiles", 1, 200, 256, 64, 128, x3=True),
    D("x3 128-wide Cout=192", 1, 200, 256, 64, 192, x3=True),
    D("x3 K=32", 1, 64, 128, 32, 64, x3=True),
    D("x3 K=64", 1, 64, 128, 64, 64, x3=True),
    D("x3 Cin=48", 1, 64, 128, 48, 64, k=3, x3=True),
    D("x3 pixel shuffle", 1, 64, 128, 64, 256, x3=True, ps2=True),
    # few output channels: the 32-wide tile from 2^16 rows (or with pre-split activations), 8 <= Cout <= 32
    D("x3 Cout=32 M=65536", 1, 256, 256, 64, 32, x3=True),
    D("x3 Cout=32 M=65535", 1, 1, 65535, 64, 32, x3=True),
    D("x3 Cout=8 M=65536", 1, 256, 256, 64, 8, x3=True),
    D("x3 Cout=7 M=65536", 1, 256, 256, 64, 7, x3=True),
    D("x3 Cout=33 M=65536", 1, 256, 256, 64, 36, x3=True),
    D("x3 Cout=63 M=65536", 1, 256, 256, 64, 60, x3=True),
    # tail split of the 256-wide tile: last round <= 64 of 256 tiles
    D("x3 320 tiles: last round 64", 1, 320, 256, 64, 256, x3=True),
    D("x3 321 tiles: last round 65", 1, 321, 256, 64, 256, x3=True),
    D("x3 258 tiles + tail", 1, 129, 256, 64, 512, x3=True),
    # ---- K >= 1152: the hand-pipelined tiles, run-staged for 3 x 3 stride-1 "same" layers
    D("x3 K=1120", 1, 256, 256, 1120, 256, x3=True),
    D("x3 K=1152 pipe", 1, 256, 256, 1152, 256, x3=True),
    D("x3 run3 256", 1, 256, 256, 128, 256, k=3, x3=True),
    D("x3 run3 256 window, batch", 2, 128, 256, 128, 256, k=3, x3=True, cs=192, in_coff=32),
    D("x3 run3 128", 1, 200, 256, 128, 128, k=3, x3=True),
    D("x3 pipe 256 stride 2", 1, 512, 512, 128, 256, k=3, stride=2, x3=True),
    D("x3 pipe 128 stride 2", 1, 400, 512, 128, 128, k=3, stride=2, x3=True),
    D("x3 128-wide Cout=192 long K", 1, 200, 256, 128, 192, k=3, x3=True),
    D("x3 run3 + tail", 1, 129, 256, 128, 512, k=3, x3=True),
    D("x3 pipe + tail", 1, 258, 512, 128, 512, k=3, stride=2, x3=True),
    D("x3 31 taps", 1, 230, 256, 64, 128, k=(31, 1), x3=True),
    D("x3 32 taps", 1, 231, 256, 64, 128, k=(32, 1), x3=True),
    D("x3 33 taps", 1, 232, 256, 64, 128, k=(33, 1), x3=True),
    # ---- pre-split activations / pair-format output
    D("pair M=2048", 1, 32, 64, 64, 64, k=3, x3=True, in_pair=True),
    D("pair M=2047", 1, 1, 2047, 64, 64, x3=True, in_pair=True),
    D("pair Cout=8", 1, 64, 128, 64, 8, k=3, x3=True, in_pair=True),
    D("pair Cout=4", 1, 64, 128, 64, 4, k=3, x3=True, in_pair=True),
    D("pair Cout=32", 1, 64, 128, 64, 32, k=3, x3=True, in_pair=True, out_pair=True),
    D("pair Cout=48", 1, 64, 128, 64, 48, k=3, x3=True, in_pair=True),
    D("pair 64-wide", 1, 64, 128, 64, 64, k=3, x3=True, in_pair=True),
    D("pair 128-wide", 1, 200, 256, 32, 128, k=3, x3=True, in_pair=True),
    D("pair 256-wide", 1, 256, 256, 64, 256, x3=True, in_pair=True),
    D("pair 256-wide + tail", 1, 129, 256, 64, 512, x3=True, in_pair=True),
    D("pair run3 256", 1, 256, 256, 128, 256, k=3, x3=True, in_pair=True),
    D("pair run3 128", 1, 200, 256, 128, 128, k=3, x3=True, in_pair=True),
    D("pair pipe 256", 1, 512, 512, 128, 256, k=3, stride=2, x3=True, in_pair=True),
    D("pair pipe 128", 1, 400, 512, 128, 128, k=3, stride=2, x3=True, in_pair=True),
    D("pair run3 + tail", 1, 129, 256, 128, 512, k=3, x3=True, in_pair=True),
    D("pair window off the 16-channel groups", 1, 64, 128, 64, 64, k=3, x3=True, in_pair=True, cs=96, in_coff=8),
    D("out_pair only", 1, 64, 128, 64, 64, k=3, x3=True, out_pair=True),
    D("pair Cin=48", 1, 64, 128, 48, 64, k=3, x3=True, in_pair=True),
    # ---- split-K: the caller asks for rows <= 4096, K >= 2048
    D("x3 split-K M=3136 3x3", 8, 14, 28, 512, 512, k=3, x3=True),
    D("x3 split-K M=512", 16, 4, 8, 512, 512, k=3, x3=True),
    D("x3 split-K M=511", 1, 1, 511, 2048, 512, x3=True),
    D("x3 split-K Cout=64", 1, 1, 512, 2048, 64, x3=True),
    D("x3 split-K Cout=60", 1, 1, 512, 2048, 60, x3=True),
    D("x3 split-K 240 tiles", 1, 64, 64, 2048, 960, x3=True),
    D("x3 split-K 256 tiles", 1, 64, 64, 2048, 1024, x3=True),
    D("x3 K=2032: not asked", 1, 1, 512, 2032, 512, x3=True),
    D("igemm split-K 128-wide", 1, 1, 64, 2048, 128),
    D("igemm split-K 64-wide", 1, 1, 64, 2048, 48),
    D("igemm split-K 32-wide", 1, 1, 64, 2048, 16),
    D("igemm split-K 16-bit", 1, 1, 64, 2048, 128, dt="f16"),
    D("igemm atomic split-K 127 tiles", 1, 1, 127 * 128, 128, 128, ws=True),
    D("igemm 128 tiles: no split", 1, 1, 128 * 128, 128, 128, ws=True),
    D("igemm atomic split-K 8 K tiles", 1, 1, 300, 128, 64, ws=True),
    D("igemm 7 K tiles: no split", 1, 1, 300, 112, 64, ws=True),
    D("x3 operand, atomic workspace", 8, 14, 28, 512, 512, k=3, x3=True, ws=True),
    # ---- exact f32 on the LDS-DMA kernel (Cin % 16, Cout >= 64) and the register-staged kernel
    D("f32 glds 64-wide", 1, 64, 128, 16, 64, k=3),
    D("f32 glds 128-wide", 1, 64, 128, 16, 65 + 3, k=3),
    D("f32 glds K=16", 1, 64, 128, 16, 64),
    D("f32 Cout=63", 1, 64, 128, 16, 60, k=3),
    D("igemm 128-wide Cin=8", 1, 64, 128, 8, 128, k=3),
    D("igemm 64-wide Cin=8", 1, 64, 128, 8, 33 + 3, k=3),
    D("igemm 32-wide Cin=8", 1, 64, 128, 8, 32, k=3),
    D("igemm Cout=7", 1, 64, 128, 8, 7, k=3),
    D("f32 M=2047", 1, 1, 2047, 64, 2080),
    # ---- 16-bit operands on the LDS-DMA kernel: the four tiles of Cout > 64, the two 64-wide ones, the tail split
    D("bf16 256-wide 128 B rows, 200 tiles", 1, 200, 256, 64, 256, dt="bf16"),
    D("bf16 199 tiles, K <= 512", 1, 199, 256, 64, 256, dt="bf16"),
    D("bf16 256-wide 64 B rows", 1, 200, 256, 32, 256, k=3, dt="bf16"),
    D("bf16 K=576", 1, 64, 128, 64, 128, k=3, dt="bf16"),
    D("bf16 K=512", 1, 64, 128, 512, 128, dt="bf16"),
    D("bf16 K=544", 1, 64, 128, 544, 128, dt="bf16"),
    D("bf16 + tail", 1, 129, 256, 64, 512, dt="bf16"),
    D("f16 + tail", 1, 129, 256, 64, 512, dt="f16"),
    D("f16 256-wide 128 B rows", 1, 200, 256, 64, 256, dt="f16"),
    D("bf16 64-wide 128 B rows", 1, 64, 128, 64, 64, k=3, dt="bf16"),
    D("bf16 64-wide 64 B rows", 1, 64, 128, 32, 64, k=3, dt="bf16"),
    D("f16 64-wide 64 B rows", 1, 64, 128, 32, 64, k=3, dt="f16"),
    D("bf16 Cin=16", 1, 64, 128, 16, 64, k=3, dt="bf16"),
    D("bf16 Cout=56", 1, 64, 128, 64, 56, k=3, dt="bf16"),
    D("bf16 Cout=24", 1, 64, 128, 64, 24, k=3, dt="bf16"),
    D("bf16 K=32", 1, 64, 128, 32, 64, dt="bf16"),
    D("bf16 M=2047", 1, 1, 2047, 64, 2080, dt="bf16"),
    D("bf16 row-run stem", 6, 70, 104, 64, 64, k=(7, 1), stride=2, pad=0, dt="bf16", cs=8, in_cstride=8, out_hw=(32, 48)),
    # ---- sparse: the three run kernels (stride 1, 27 taps, Cin % 32, Cout 32 / 64 / 128), else the gathered LDS-DMA tiles
    S("sparse runs 32", 3200, 32, 32, x3=True),
    S("sparse runs 64", 3200, 64, 64, x3=True),
    S("sparse runs 128", 3200, 128, 128, x3=True),
    S("sparse runs M=2048", 2048, 32, 32, x3=True),
    S("sparse M=2047", 2047, 32, 32, x3=True),
    S("sparse stride 2", 3200, 32, 64, stride=2, x3=True),
    S("sparse tile plan", 3200, 32, 32, x3=True, plan=True),
    S("sparse x3 Cin=16 Cout=32", 3200, 16, 32, x3=True),
    S("sparse x3 Cout=48", 3200, 32, 48, x3=True),
    S("sparse x3 Cout=96", 3200, 32, 96, x3=True),
    S("sparse x3 Cout=16", 3200, 32, 16, x3=True),
    S("sparse x3 Cout=12", 3200, 32, 12, x3=True),
    S("sparse x3 Cout=132", 3200, 32, 132, x3=True),
    S("sparse f32", 3200, 32, 32),
    S("sparse bf16 32", 3200, 32, 32, dt="bf16"),
    S("sparse bf16 64", 3200, 32, 64, dt="bf16"),
    S("sparse bf16 128", 3200, 32, 128, dt="bf16"),
    S("sparse f16 32", 3200, 32, 32, dt="f16"),
    S("sparse f16 64", 3200, 64, 64, dt="f16"),
    S("sparse f16 128", 3200, 64, 128, dt="f16"),
    S("sparse bf16 Cin=48", 3200, 48, 64, dt="bf16"),
    S("sparse bf16 tile plan", 3200, 32, 64, dt="bf16", plan=True),
]


# Asked directly, never launched: both sides of the bounds of the bf16x3 split-K tile (512 <= M <= 8192, K >= 1024, < 256 tiles, at
# most 32 taps, no pixel shuffle) that the caller's own gate keeps ops.conv2d away from, each with the workspace the answer sizes.
QUERIES = [dict(c, ask=True) for c in [
    D("query x3 M=8192", 1, 64, 128, 1024, 448, x3=True),
    D("query x3 M=8193", 1, 1, 8193, 1024, 448, x3=True),
    D("query f32 M=8192", 1, 64, 128, 1024, 448),
    D("query x3 K=1024", 1, 1, 512, 1024, 512, x3=True),
    D("query x3 K=992", 1, 1, 512, 992, 512, x3=True),
    D("query x3 255 tiles", 1, 1, 3840, 1024, 1088, x3=True),
    D("query x3 256 tiles", 1, 1, 4096, 1024, 1024, x3=True),
    D("query x3 32 taps", 1, 40, 64, 32, 512, k=(32, 1), x3=True),
    D("query x3 33 taps", 1, 40, 64, 32, 512, k=(33, 1), x3=True),
    D("query x3 pixel shuffle", 1, 1, 512, 1024, 512, x3=True, ps2=True),
]]


def _fields():
    from thinktwice_amd import ops
    return [(n, t is ctypes.c_void_p) for n, t in ops._ConvDesc._fields_]


def desc_to_dict(d):
    return {n: (int(bool(getattr(d, n))) if is_ptr else int(getattr(d, n))) for n, is_ptr in _fields()}


def dict_to_desc(row):
    """A recorded row as a descriptor ops.plan_label takes: dummy 64-byte aligned addresses where the row has a pointer."""
    from thinktwice_amd import ops
    d = ops._ConvDesc()
    for i, (n, is_ptr) in enumerate(_fields()):
        if is_ptr:
            setattr(d, n, 0x10000 * (i + 1) if row.get(n) else None)
        else:
            setattr(d, n, row.get(n, 0))
    return d


def plan_label(L, d):
    """ops.plan_label(d), under the name and signature this tool's other users call (L: the loaded library, not needed any more)."""
    from thinktwice_amd import ops
    return ops.plan_label(d)


def _strides(shape):
    """Element strides of a contiguous tensor of this shape."""
    st = [1]
    for n in reversed(shape[1:]):
        st.insert(0, st[0] * n)
    return tuple(st)


def describe(c, L):
    """The descriptor ops.conv2d / ops.gather_conv build for a case (pointers 1 / 0), and the split-K query's answer where they ask."""
    from thinktwice_amd import ops
    here = lambda flag: 1 if flag else None       # the "address" of an operand the case has
    operands = dict(x=1, w=1, out=1, dtype=DT[c["dt"]], out_dtype=DT[c["dt"]], weight_x3=here(c["x3"]))
    if c["kind"] == "sparse":
        d = ops.conv_desc(x_shape=(GRID[0] * GRID[1] * GRID[2] * GRID[3], c["Cin"]), x_strides=None, w_shape=(c["Cout"], 1, 27, c["Cin"]),
                          out_shape=(c["M"], c["Cout"]), out_strides=None, stride=c["stride"], shift_n_mod=0, gather=(1, 1, c["M"]),
                          plan=(1, 1) if c["plan"] else None, **operands)
        return desc_to_dict(d), None
    x_shape, w_shape = (c["N"], c["H"], c["W"], c["cs"]), (c["Cout"], c["KH"], c["KW"], c["Cin"])
    geometry = dict(stride=c["stride"], pad=c["pad"], out_hw=c["out_hw"], pixel_shuffle2=c["ps2"])
    _, _, OH, OW, out_shape = ops.conv_geometry(x_shape, w_shape, **geometry)
    full = (c["N"], OH, OW, c["Cout"])       # the shape of a residual and of the second output
    d = ops.conv_desc(x_shape=x_shape, x_strides=_strides(x_shape), w_shape=w_shape, out_shape=out_shape, out_strides=_strides(out_shape),
                      in_coff=c["in_coff"], in_cstride=c["in_cstride"], res1=here(c["res"] >= 1), res1_shape=full, res1_dtype=DT[c["dt"]],
                      res2=here(c["res"] >= 2), res2_shape=full, weight_h2=here(c["h2"]), in_pair=c["in_pair"], out_pair=c["out_pair"],
                      out2=here(c["out2"]), out2_shape=full, **geometry, **operands)
    row = desc_to_dict(d)
    query = None
    if c.get("ask") or ops.auto_splitk_asks(c["N"] * OH * OW, c["KH"] * c["KW"] * c["Cin"], splitk_ws=c["ws"],
                                            pair=c["in_pair"] or c["out_pair"], h2=c["h2"]):
        query = int(L.tt_conv2d_splitk_slices(ctypes.byref(dict_to_desc(row))))
    if c["ws"] or query:
        row.update(splitk_ws=1, splitk_slices=query or 0)
    return row, query


def _lib_only():
    from thinktwice_amd import _lib
    return _lib.lib()


def run_plan(cases=None):
    from thinktwice_amd import _lib, ops
    L = _lib.lib()
    out = []
    for c in cases or CASES + QUERIES:
        row, query = describe(c, L)
        rec = dict(name=c["name"], desc=row, label=ops.plan_label(dict_to_desc(row)))
        if query is not None:
            rec["query"] = query
        out.append(rec)
    return out


def _grid_rulebook(dims):
    """Rulebook of a 3x3x3 SubM conv on a fully occupied grid, rows in (b, z, y, x) cell order like csrc/lidar.hip builds them."""
    import torch
    import torch.nn.functional as F
    B, Dz, H, W = dims
    idx = torch.arange(B * Dz * H * W).view(B, Dz, H, W)
    pad = F.pad(idx, (1, 1, 1, 1, 1, 1), value=-1)
    b, z, y, x = torch.ones(dims, dtype=torch.bool).nonzero().unbind(1)
    taps = [pad[b, z + kz, y + ky, x + kx] for kz in range(3) for ky in range(3) for kx in range(3)]
    return torch.stack(taps, 1).to(torch.int32)


def run_launch(cases=None):
    import torch
    from thinktwice_amd import _lib, ops
    L = _lib.lib()
    real = L.tt_conv2d_fwd
    seen = {}

    def spy(d, stream):          # d = byref(_ConvDesc): keep what the library was handed
        seen["desc"] = desc_to_dict(d._obj)
        return real(d, stream)
    L.tt_conv2d_fwd = spy
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    nbr_full = _grid_rulebook(GRID).cuda()
    out = []
    for c in cases or CASES + QUERIES:
        want, query = describe(c, L)
        if c.get("ask"):
            out.append(dict(name=c["name"], desc=want, query=query))
            continue
        dt = tdt[c["dt"]]
        z = lambda *shape, dtype=dt: torch.zeros(*shape, dtype=dtype, device="cuda")
        try:
            if c["kind"] == "sparse":
                nbr = nbr_full[:c["M"]].contiguous()
                m_dev = torch.tensor([c["M"]], dtype=torch.int32, device="cuda")
                w = z(c["Cout"], 1, 27, c["Cin"])
                ops.gather_conv(z(nbr_full.shape[0], c["Cin"]), nbr, m_dev, w, w_x3=torch.zeros_like(w) if c["x3"] else None,
                                plan=ops.sp_tile_plan(nbr, m_dev) if c["plan"] else None, stride=c["stride"])
            else:
                w = z(c["Cout"], c["KH"], c["KW"], c["Cin"])
                M = want["N"] * want["OH"] * want["OW"]
                res = [z(want["N"], want["OH"], want["OW"], c["Cout"]) for _ in range(c["res"])]
                ops.conv2d(z(c["N"], c["H"], c["W"], c["cs"]), w, stride=c["stride"], pad=c["pad"], in_coff=c["in_coff"], cin=c["Cin"],
                           pixel_shuffle2=c["ps2"], w_x3=torch.zeros_like(w) if c["x3"] else None,
                           w_h2=z(c["Cout"], c["KH"], c["KW"], 2 * c["Cin"]) if c["h2"] else None, in_pair=c["in_pair"],
                           out_pair=c["out_pair"], splitk_ws=z(M, c["Cout"], dtype=torch.float32) if c["ws"] else None,
                           in_cstride=c["in_cstride"], out_hw=c["out_hw"], res1=res[0] if res else None, res2=res[1] if res[1:] else None,
                           out2=z(want["N"], want["OH"], want["OW"], c["Cout"], dtype=torch.float32) if c["out2"] else None)
            torch.cuda.synchronize()
            label = ops._last_conv_kernel()
        except _lib.TTError as e:
            label = "ERROR: " + str(e).split("): ", 1)[1]
        got = seen.pop("desc")
        assert got == want, (c["name"], {k: (got[k], want[k]) for k in got if got[k] != want[k]})
        rec = dict(name=c["name"], desc=got, label=label)
        if query is not None:
            rec["query"] = query
        out.append(rec)
    L.tt_conv2d_fwd = real
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--launch", action="store_true")
    g.add_argument("--plan", action="store_true")
    g.add_argument("--query", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    cases = run_launch() if a.launch else run_plan() if a.plan else [dict(name=c["name"], desc=r, query=q) for c in QUERIES
                                                                      for r, q in [describe(c, _lib_only())]]
    for c in cases:
        c["desc"] = {k: v for k, v in c["desc"].items() if v}
    text = "{\"cases\": [\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]}\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    else:
        sys.stdout.write(text)
    print(f"{len(cases)} cases, {len({c['label'] for c in cases if 'label' in c})} distinct labels", file=sys.stderr)


if __name__ == "__main__":
    main()
