"""Thin tensor->pointer wrappers over the C ABI (include/thinktwice_hip.h).

All functions take device tensors and launch on torch's current stream.  No function here
computes anything in PyTorch: allocation and stream handling only.
"""
import contextlib
import ctypes
import functools
import math
import os

import torch

from . import _lib
from ._lib import (TT_BF16, TT_F16, TT_F32, TTError, check, clear_device_faults, cur_stream, device_faults, lib, ptr,  # noqa: F401
                   raise_on_device_fault, require_cuda)
# The only reference to the training tape.  autodiff imports this module in turn; whichever of the two is imported first sees the
# other half-initialised, which is fine because neither touches the other at import time: autodiff.TAPE is read per call.
from . import autodiff


def _active_tape():
    """The tape that records this call's backward (autodiff.TAPE, read at call time: the trainer and the tests assign to it)."""
    return autodiff.TAPE


def _tape(op, *args):
    """The tape hook of every differentiable wrapper: TAPE.<op>(*args) while a tape is active, nothing otherwise."""
    tape = _active_tape()
    if tape is not None:
        getattr(tape, op)(*args)


def _st(t):
    """The current stream of this tensor's device."""
    return cur_stream(t.device)


def _cs(t):
    """Channel stride (the last dimension) of an optional channel-last operand."""
    return 0 if t is None else t.shape[-1]


def _workspace(nbytes, device):
    """Scratch bytes for one launch, sized by the entry's own *_workspace_bytes query."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def _level_hw(level_hw):
    """(H, W) of the four feature levels as the int[8] the look-module entries take."""
    return (ctypes.c_int * 8)(*[v for pair in level_hw for v in pair])


def dtype_code(t):
    if t.dtype == torch.float32:
        return TT_F32
    if t.dtype == torch.bfloat16:
        return TT_BF16
    if t.dtype == torch.float16:
        return TT_F16
    raise _lib.TTError(f"unsupported dtype {t.dtype}")


def frustum_voxel_index(frustum, mats, voxel_lo, voxel_size, batch_size, num_cams, want_f32=False):
    """frustum [D,fH,fW,4] f32 (device); mats [B*ncam,2,4,4] f32 (device): inv(ida), s2e@inv(K).
    voxel_lo / voxel_size: 3 python floats each.  -> geom_xyz int32 [B, ncam*D*fH*fW, 3]."""
    require_cuda(frustum, mats)
    assert frustum.is_contiguous() and mats.is_contiguous()
    D, fH, fW, _ = frustum.shape
    geom = torch.empty(batch_size, num_cams * D * fH * fW, 3, dtype=torch.int32, device=frustum.device)
    gf = torch.empty(geom.shape, dtype=torch.float32, device=frustum.device) if want_f32 else None
    lo = (ctypes.c_float * 3)(*[float(v) for v in voxel_lo])
    sz = (ctypes.c_float * 3)(*[float(v) for v in voxel_size])
    rc = lib().tt_frustum_voxel_index(batch_size, num_cams, D, fH, fW, ptr(frustum), ptr(mats), lo, sz, ptr(geom), ptr(gf),
                                      _st(frustum))
    check(rc, "tt_frustum_voxel_index")
    return (geom, gf) if want_f32 else geom


_LIFT_SPLAT_ATOMIC = os.environ.get("TT_LIFT_SPLAT_ATOMIC", "0") == "1"


def lift_splat(depth_logits, context, geom_xyz, voxel_num, batch_size, num_cams, out=None,
               out_coff=0, rot_flip=False, record=True):
    """depth_logits [B*ncam,fH,fW,D], context [B*ncam,fH,fW,C] (channel-last, f32 or bf16),
    geom_xyz int32 [B, ncam*D*fH*fW, 3] -> out f32 [B, Y, X, Ctot] (accumulated into `out`)."""
    require_cuda(depth_logits, context, geom_xyz)
    assert depth_logits.is_contiguous() and context.is_contiguous() and geom_xyz.is_contiguous()
    BN, fH, fW, D = depth_logits.shape
    C = context.shape[-1]
    vx, vy, vz = (int(v) for v in voxel_num)
    if out is None:
        oh, ow = (vx, vy) if rot_flip else (vy, vx)
        out = torch.zeros(batch_size, oh, ow, C, dtype=torch.float32, device=context.device)
    # workspace form: (strip, cell) partial rows + an ordered per-cell reduce instead of f32 atomics (bit-reproducible);
    # TT_LIFT_SPLAT_ATOMIC=1 selects the single-kernel atomic form for A/B
    ws, ws_bytes = None, 0
    if not _LIFT_SPLAT_ATOMIC:
        ws_bytes = int(lib().tt_lift_splat_workspace_bytes(batch_size, num_cams, D, fH, fW, C, vx, vy))
        if ws_bytes > 0:
            ws = _workspace(ws_bytes, context.device)
    rc = lib().tt_lift_splat_fwd_ws(batch_size, num_cams, D, fH, fW, C, vx, vy, vz, ptr(depth_logits), ptr(context),
                                    dtype_code(context), ptr(geom_xyz), ptr(out), out.shape[-1], out_coff, 1 if rot_flip else 0,
                                    ptr(ws), ws_bytes, _st(context))
    check(rc, "tt_lift_splat_fwd_ws")
    if record:
        _tape("lift_splat", depth_logits, context, geom_xyz, (vx, vy, vz), batch_size, num_cams, out, out_coff, rot_flip)
    return out


def lift_splat_bwd(depth_logits, context, geom_xyz, voxel_num, batch_size, num_cams, gout, out_coff, gdepth, gctx):
    """gdepth += , gctx += backward of lift_splat (f32; gout: the BEV gradient buffer [B, Y, X, Ctot])."""
    require_cuda(depth_logits, context, geom_xyz, gout, gdepth, gctx)
    BN, fH, fW, D = depth_logits.shape
    C = context.shape[-1]
    vx, vy, vz = voxel_num
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (depth_logits, context, gout, gdepth, gctx))
    check(lib().tt_lift_splat_bwd(batch_size, num_cams, D, fH, fW, C, vx, vy, vz,
                                  ptr(depth_logits), ptr(context), ptr(geom_xyz), ptr(gout), gout.shape[-1],
                                  out_coff, ptr(gdepth), ptr(gctx), _st(context)), "tt_lift_splat_bwd")


# ----------------------------------------------------------------------------- conv / linear
_AUTO_SPLITK = os.environ.get("TT_CONV_AUTO_SPLITK", "1") == "1"
SMALL_ROWS = _lib.TT_CONV_SMALL_ROWS    # up to this many output rows a plain layer runs the exact-f32 latency kernel (conv_choose.cpp, choose_small)
CONV_PROFILE = None   # bench.py sets this to a list to collect (flops, start, end, shape) per launch
CONV_KERNELS = None   # same order as CONV_PROFILE: tt_conv_last_kernel() of the launch (a weight gradient: its plan label); plus one
                      # entry per gather_conv_wgrad, which has no CONV_PROFILE record -- do not zip the two over a sparse backward
CONV_BYTES = None     # same order as CONV_PROFILE: compulsory HBM bytes of the launch (each operand moved once);
                      # dense: int; sparse: (bytes per live output row, fixed bytes)

_ConvDesc = _lib.structs()["tt_conv_desc"]      # `in` is spelled `in_`
_ConvNext = _lib.structs()["tt_conv_next"]      # the joined stage of tt_conv2d_fwd_next


def _last_conv_kernel():
    L = lib()
    return L.tt_conv_last_kernel().decode()


class _Launch:
    """The launch recorder of the convolution wrappers:

        with _launch() as rec:
            check(lib().tt_...(...))
        if rec is not None:
            rec.log(flops, shape, kernel=..., nbytes=...)

    While the bench collects (CONV_PROFILE is a list) the block runs between two timing events and `log` files the launch in the
    three lists; otherwise `_launch()` hands out the shared idle recorder: `rec` is None, no event, no label query."""

    def __enter__(self):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.e0.record()
        return self

    def __exit__(self, *exc):
        self.e1.record()

    def log(self, flops, shape, *sparse, kernel, nbytes):
        """CONV_PROFILE gets (flops, start, end, shape) -- a sparse launch adds its three (m_dev, M, per-row taps) entries;
        CONV_KERNELS the label: a string, or a function asked only when the list is kept; CONV_BYTES `nbytes`."""
        CONV_PROFILE.append((flops, self.e0, self.e1, shape) + sparse)
        if CONV_KERNELS is not None:
            CONV_KERNELS.append(kernel if isinstance(kernel, str) else kernel())
        if CONV_BYTES is not None:
            CONV_BYTES.append(nbytes)


_IDLE = contextlib.nullcontext()      # `with _IDLE as rec`: rec is None


def _launch():
    return _IDLE if CONV_PROFILE is None else _Launch()


def conv_geometry(x_shape, w_shape, stride=1, pad=0, dil=1, out_hw=None, pixel_shuffle2=False, in_up2=False):
    """The sizes of a dense convolution, from plain numbers: (H, W, OH, OW, out_shape).  H, W: the logical input (in_up2: the
    upsampled map, twice the source tensor's); OH, OW: the usual formula, or `out_hw` where the caller states them (row-run form);
    out_shape: the tensor the layer writes when it allocates it (pixel_shuffle2: the four channel groups spread 2 x 2)."""
    N, H, W, _ = x_shape
    if in_up2:
        H, W = 2 * H, 2 * W
    Cout, KH, KW, _ = w_shape
    OH = (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1
    OW = (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1
    if out_hw is not None:
        OH, OW = out_hw
    return H, W, OH, OW, ((N, 2 * OH, 2 * OW, Cout // 4) if pixel_shuffle2 else (N, OH, OW, Cout))


def conv_desc(x, x_shape, x_strides, w, w_shape, out, out_shape, out_strides, dtype, out_dtype,
              stride=1, pad=0, dil=1, out_hw=None, pixel_shuffle2=False, in_up2=False,
              in_coff=0, in_cstride=None, out_coff=0, out_nstride=0,
              scale=None, shift=None, shift_n=None, shift_n_mod=1, act=0,
              res1=None, res1_shape=None, res1_dtype=None, res1_coff=0, res1_up=False, res2=None, res2_shape=None, res2_coff=0,
              weight_x3=None, weight_h2=None, in_pair=False, out_pair=False, out2=None, out2_shape=None, out2_coff=0,
              gather=None, plan=None):
    """The filled tt_conv_desc of one launch, from plain numbers: no tensor comes in.  x / w / out / scale / shift / shift_n /
    res1 / res2 / weight_x3 / weight_h2 / out2: element addresses (int, None = absent); *_shape / *_strides: the tensors' own, in
    elements; dtype / out_dtype / res1_dtype: TT_F32 / TT_BF16 / TT_F16 (res1_dtype None: the operands'); the rest as conv2d names them.
    gather = (rulebook address, m_dev address, M) makes it the sparse form of gather_conv -- x_shape [R_in, Cin] rows, one "pixel"
    per output row, the taps along KW, `stride` only a hint to the dispatch -- and plan = (row_perm, row_mask) addresses its tile plan.
    The split-K fields are the caller's to set once the library has answered the query about this descriptor.
    The signature has one line per group.  conv2d, which runs a few hundred times per forward, passes the groups by position, line
    for line (matching forty keywords costs more than filling the forty fields): whoever moves a parameter moves it there too."""
    Cout, KH, KW, Cin = w_shape
    if gather is None:
        N, Cs = x_shape[0], x_shape[3]
        H, W, OH, OW, _ = conv_geometry(x_shape, w_shape, stride, pad, dil, out_hw, pixel_shuffle2, in_up2)
        in_nstride = x_strides[0] if N > 1 else 0        # one image: no batch stride to trust
        out_nstride = out_nstride or (out_strides[0] if (len(out_shape) == 4 and N > 1) else 0)
    else:
        N, Cs = gather[2], x_shape[1]
        H = W = OH = OW = 1
        in_nstride = out_nstride = 0
    d = _ConvDesc()         # all zeroes: an absent operand or an unused mode below leaves its fields so
    d.in_ = x; d.N = N; d.H = H; d.W = W; d.Cin = Cin; d.in_cstride = in_cstride or Cs; d.in_coff = in_coff
    d.in_nstride = in_nstride
    d.weight = w; d.Cout = Cout; d.KH = KH; d.KW = KW; d.stride = stride; d.pad = pad; d.dil = dil
    d.out = out; d.OH = OH; d.OW = OW
    d.out_cstride = out_shape[-1]; d.out_coff = out_coff
    d.out_nstride = out_nstride
    d.act = act; d.dtype = dtype; d.out_dtype = out_dtype
    d.shift_n_mod = shift_n_mod
    if scale is not None:
        d.scale = scale
    if shift is not None:
        d.shift = shift
    if shift_n is not None:
        d.shift_n = shift_n
    d.res1_coff = res1_coff
    if res1 is not None:
        d.res1 = res1; d.res1_cstride = res1_shape[-1]
        if res1_dtype == TT_F32 and dtype != TT_F32:
            d.res1_f32 = 1              # an f32 sum chain beside half conv inputs (mixed mode's PAFPN)
    if res1_up:                         # res1 is the coarser map, added through nearest upsampling
        d.res1_up_h, d.res1_up_w = res1_shape[1], res1_shape[2]
    d.res2_coff = res2_coff
    if res2 is not None:
        d.res2 = res2; d.res2_cstride = res2_shape[-1]
    if out2 is not None:
        d.out2 = out2; d.out2_cstride = out2_shape[-1]; d.out2_coff = out2_coff
    if weight_x3 is not None:
        d.weight_x3 = weight_x3
    if weight_h2 is not None:
        d.weight_h2 = weight_h2
    if pixel_shuffle2:
        d.pixel_shuffle2 = 1
    if in_pair:
        d.in_pair = 1
    if out_pair:
        d.out_pair = 1
    if in_up2:
        d.in_up2 = 1
    if gather is not None:
        d.gather_idx, d.m_dev = gather[0], gather[1]
    if plan is not None:
        d.row_perm, d.row_mask = plan
    return d


SPARSE_PAIRS = None   # bench.py: device int64 counter of existing (row, tap) pairs, filled by sp_tile_plan


def sp_tile_plan(nbr, m_dev):
    """Tile plan of a rulebook (tt_sp_tile_plan): (row_perm int32 [M], row_mask int32-typed uint32 [M]) -- the output
    rows sorted by tap-occupancy mask, so that a 256-row tile of the gathered GEMM only visits the union of its taps."""
    require_cuda(nbr, m_dev)
    M, KV = nbr.shape
    ws = _workspace(lib().tt_sp_tile_plan_workspace_bytes(M), nbr.device)
    perm = torch.empty(M, dtype=torch.int32, device=nbr.device)
    mask = torch.empty(M, dtype=torch.int32, device=nbr.device)
    check(lib().tt_sp_tile_plan(ptr(nbr), ptr(m_dev), M, KV, ptr(ws), ws.numel(), ptr(perm), ptr(mask),
                                ptr(SPARSE_PAIRS), _st(nbr)), "tt_sp_tile_plan")
    return perm, mask


def gather_conv(feats, nbr, m_dev, w, *, scale=None, shift=None, act=0, res=None, out_dtype=None, w_x3=None, plan=None,
                out=None, in_rows=None, stride=1, _no_tape=False, bn_raw=False):
    """Sparse convolution as a gathered GEMM on MFMA: feats [R_in, C] rows, nbr int32 [M, taps]
    (rulebook, -1 = no input), m_dev device int (live output rows), w [Cout,1,taps,C] -> [M, Cout].  `stride`: the spatial
    stride of the sparse conv the rulebook came from (a dispatch hint: stride-1 rulebooks of cell-ordered rows take the
    run-staged kernel, csrc/sp_conv_runs.hip; the arithmetic does not depend on it)."""
    require_cuda(feats, nbr, w)
    M, taps = nbr.shape
    Cout, _, KW, Cin = w.shape
    assert KW == taps and feats.shape[1] == Cin and feats.is_contiguous() and nbr.is_contiguous()
    if out is None:
        out = torch.empty(M, Cout, dtype=out_dtype or feats.dtype, device=feats.device)
    assert tuple(out.shape) == (M, Cout) and out.is_contiguous()
    d = conv_desc(x=feats.data_ptr(), x_shape=feats.shape, x_strides=None, w=w.data_ptr(), w_shape=(Cout, 1, KW, Cin),
                  out=out.data_ptr(), out_shape=out.shape, out_strides=None, dtype=dtype_code(feats), out_dtype=dtype_code(out),
                  stride=stride, scale=ptr(scale), shift=ptr(shift), shift_n_mod=0, act=act, res1=ptr(res),
                  res1_shape=None if res is None else res.shape, weight_x3=ptr(w_x3), gather=(nbr.data_ptr(), ptr(m_dev), M),
                  plan=None if plan is None else (plan[0].data_ptr(), plan[1].data_ptr()))
    with _launch() as rec:
        check(lib().tt_conv2d_fwd(ctypes.byref(d), _st(feats)), "tt_conv2d_fwd(gather)")
    if rec is not None:
        esz, osz = feats.element_size(), out.element_size()
        # FLOP accounting over the EXISTING (row, tap) pairs: per-row tap counts of the rulebook (measurement only)
        # bytes: one input row and one output row (+ residual row) per live output row, rulebook row
        rec.log(2.0 * Cout * KW * Cin, f"sparse M<={M} N={Cout} K={KW * Cin}", m_dev, M, ((nbr >= 0).sum(1), 2.0 * Cout * Cin),
                kernel=_last_conv_kernel,
                nbytes=(Cin * esz + Cout * osz + (Cout * esz if res is not None else 0) + KW * 4, w.numel() * w.element_size()))
    if not _no_tape:
        _tape("gather_conv", feats, nbr, m_dev, w, scale, shift, act, res, out, in_rows, bn_raw)
    return out


def gather_conv_wgrad(feats, nbr, m_dev, dy, taps, cin_pad=None):
    """Weight gradient of gather_conv: feats [R_in, Cin] f32, nbr int32 [M, taps], dy [M, Cout] f32 -> [Cout,1,taps,cin_pad]."""
    require_cuda(feats, nbr, dy)
    M, Cout = dy.shape
    Cin = feats.shape[1]
    cin_pad = cin_pad or Cin
    out = torch.empty(Cout, 1, taps, cin_pad, dtype=torch.float32, device=dy.device)
    L = lib()
    ws = _workspace(L.tt_gather_conv_wgrad_workspace_bytes(M, Cout, Cin, cin_pad, taps), dy.device)
    assert feats.is_contiguous() and dy.is_contiguous() and nbr.is_contiguous() and feats.dtype == torch.float32
    nb = ws.numel()
    check(L.tt_gather_conv_wgrad(ptr(feats), Cin, Cin, ptr(nbr), ptr(m_dev), M, taps, ptr(dy), Cout,
                                 Cout, cin_pad, 0, ptr(out), ptr(ws), nb, _st(dy)), "tt_gather_conv_wgrad")
    if CONV_KERNELS is not None:      # (no CONV_PROFILE record goes with it: this launch is not timed, so not under _launch())
        label = ctypes.create_string_buffer(192)
        check(L.tt_gather_conv_wgrad_plan(ptr(feats), Cin, Cin, ptr(nbr), ptr(m_dev), M, taps, ptr(dy), Cout, Cout, cin_pad, 0,
                                          ptr(out), ptr(ws), nb, 0, label, len(label)), "tt_gather_conv_wgrad_plan")
        CONV_KERNELS.append(label.value.decode())
    return out


def sp_inverse_rulebook(nbr, m_dev, rows_in):
    """inv int32 [rows_in, taps]: inv[j][t] = m with nbr[m][t] == j, else -1 (transposed rulebook of a strided sparse conv)."""
    M, taps = nbr.shape
    inv = torch.full((rows_in, taps), -1, dtype=torch.int32, device=nbr.device)
    check(lib().tt_sp_inverse_rulebook(ptr(nbr), ptr(m_dev), M, taps, ptr(inv), _st(nbr)), "tt_sp_inverse_rulebook")
    return inv


def gather_conv_dgrad(dconv, nbr, m_dev, w, gx, in_rows=None, x3=False):
    """Input gradient of gather_conv, ADDED to gx [R_in, Cin]: dconv [M, Cout] f32 (rows beyond the live count uninitialised),
    nbr / m_dev / w [Cout,1,taps,Cin] the forward layer's.  The same gathered GEMM on the transposed rulebook with gx as its
    residual and its output -- in bf16x3 like the dense input gradients when `x3` (a submanifold layer's transposed rulebook
    is a submanifold rulebook again: the run-staged kernel takes it).  `in_rows`: None for a submanifold layer, else
    (device row count, allocated rows) of the INPUT level of a strided layer."""
    from . import weights
    if in_rows is None:     # submanifold: nbr[m][t] = j  <=>  nbr[j][taps - 1 - t] = m
        wt = w.flip(2).permute(3, 1, 2, 0).contiguous()
        return gather_conv(dconv, nbr, m_dev, wt, res=gx, out=gx, _no_tape=True, w_x3=weights.split_pairs_x3(wt) if x3 else None)
    rows_dev, rows_max = in_rows
    inv = sp_inverse_rulebook(nbr, m_dev, rows_max)
    wt = w.permute(3, 1, 2, 0).contiguous()
    return gather_conv(dconv, inv, rows_dev, wt, res=gx, out=gx, _no_tape=True, stride=2,
                       w_x3=weights.split_pairs_x3(wt) if x3 else None)


def sp_to_dense(x, coords, rows, max_rows, dims, batch_size):
    """rows [R, C] at coords (b, z, y, x) -> dense channel-last (B, H, W, C*D) (== spatial_features.view(N, C*D, H, W))."""
    D, H, W = dims
    C = x.shape[1]
    dense = torch.zeros(batch_size, H, W, C * D, dtype=x.dtype, device=x.device)
    dc = (ctypes.c_int * 3)(*dims)
    check(lib().tt_sp_to_dense(ptr(x), ptr(coords), ptr(rows), max_rows, C, dc, ptr(dense), dtype_code(x),
                               _st(x)), "tt_sp_to_dense")
    _tape("sp_to_dense", x, coords, rows, max_rows, dims, dense)
    return dense


def sp_from_dense(gdense, coords, rows, max_rows, dims, grows):
    """grows += the dense gradient gathered back to the rows (backward of sp_to_dense)."""
    D, H, W = dims
    C = grows.shape[1]
    check(lib().tt_sp_from_dense(ptr(gdense), ptr(coords), ptr(rows), max_rows, C, D, H, W,
                                 ptr(grows), _st(grows)), "tt_sp_from_dense")


# conv2d options that exist for inference layouts and fusions only, and why the tape refuses each
_INFERENCE_ONLY = (
    ("w_h2", "conv2d: half-storage (h2) layers have no backward; train in dtype torch.float32 or 'f32x3'"),
    ("in_pair / out_pair", "conv2d: pair-format activations are an inference-path layout (the tape reads f32 tensors)"),
    ("in_up2", "conv2d: in_up2 is an inference-path fusion (the tape records bilinear_up2 and the convolution apart)"),
    ("nxt", "conv2d: a joined stage is an inference-path fusion (the tape records the two convolutions apart)"),
)


def _refuse_on_tape(*used):
    """`used`: whether the call uses each option of _INFERENCE_ONLY, in its order.  Raises the first one's message under a tape."""
    if any(used) and _active_tape() is not None:
        raise TTError(next(msg for u, (_, msg) in zip(used, _INFERENCE_ONLY) if u))


def _in_training_step(no_tape):
    """Whether this conv2d call belongs to a training step: the forward under the tape, or one of the backward's recomputations and
    input-gradient convolutions, which run after the tape has closed and pass _no_tape instead."""
    return _active_tape() is not None or no_tape


def _training_x3(w_x3, cout, training):
    """The bf16x3 operand a layer runs with: (for a plain launch, for a split-K launch).  Inference uses w_x3 for both.  The gradient
    goldens were taken with the exact-f32 kernels on two kinds of layer, so a training step keeps those there: the layers with fewer
    than 64 output channels (inference runs them on the 256 x 32 bf16x3 tile) drop the operand altogether, and the few-row long-K
    layers drop it for split-K -- the split-K query must not see it, or it answers for the bf16x3 split-K tile."""
    if w_x3 is None or (training and cout < 64):
        return None, None
    return w_x3, (None if training else w_x3)


def auto_splitk_asks(rows, k, splitk_ws=False, pair=False, in_up2=False, h2=False, res1_up=False):
    """Whether conv2d asks the library for a split-K workspace of its own: few rows, very long K, none of the operand modes that
    have no split-K form, and no workspace from the caller.  TT_CONV_AUTO_SPLITK=0 disables."""
    return _AUTO_SPLITK and not splitk_ws and not (pair or in_up2) and not h2 and not res1_up and rows <= SMALL_ROWS and k >= 2048


def _auto_splitk(d, device):
    """The f32 workspace of a launch auto_splitk_asks about, if the library wants it split (d.splitk_slices is then set), else None.
    Few rows, very long K (BEV-update conv K=18720, flatten MLPs): cross-workgroup split-K with an f32 workspace
    beats conv_small.hip's in-workgroup split there (277 vs 416 us on the BEV-update conv: the direct 32 B/row
    operand loads of the small kernel waste L2 sectors on a 10 MB weight matrix).
    Ordered form (no atomics, no zero fill): one [M][Cout] slice per K split, added in index order by the finalize kernel.
    With a bf16x3 operand the layer runs the 64-wide bf16x3 tile with the K tiles dealt over workgroups
    (conv_igemm_glds.hip, x3_splitk_plan) instead of the exact-f32 register-staged kernel."""
    slices = int(lib().tt_conv2d_splitk_slices(ctypes.byref(d)))
    if slices <= 0:
        return None
    d.splitk_slices = slices
    return torch.empty(slices, d.N * d.OH * d.OW, d.Cout, dtype=torch.float32, device=device)


def _joined_stage(nxt, nxt_out, nxt_out_coff, out_shape, device):
    """The tt_conv_next of conv2d(nxt=...) and the tensor it writes: the 1 x 1 convolution over the rows of `out_shape`."""
    nw, nw_x3, nscale, nshift, nact = nxt
    N, OH, OW, Cout = out_shape
    assert nw_x3 is not None and nw.is_contiguous() and nw_x3.is_contiguous() and tuple(nw.shape[1:]) == (1, 1, Cout) \
        and nw_x3.shape == nw.shape
    nout = nxt_out if nxt_out is not None else torch.empty(N, OH, OW, nw.shape[0], dtype=torch.float32, device=device)
    assert nout.dtype == torch.float32 and nout.is_contiguous() and tuple(nout.shape[:3]) == (N, OH, OW)
    dn = _ConvNext()
    dn.next_weight = nw.data_ptr(); dn.next_weight_x3 = nw_x3.data_ptr(); dn.next_cout = nw.shape[0]
    dn.next_scale = ptr(nscale); dn.next_shift = ptr(nshift); dn.next_act = nact
    dn.next_out = nout.data_ptr(); dn.next_out_cstride = nout.shape[-1]; dn.next_out_coff = nxt_out_coff; dn.next_out_pair = 1
    return dn, nout


def conv2d(x, w, *, stride=1, pad=0, dil=1, scale=None, shift=None, act=0, res1=None, res1_coff=0,
           res2=None, res2_coff=0, out=None, out_coff=0, in_coff=0, cin=None, pixel_shuffle2=False,
           shift_n=None, shift_n_mod=1, out_dtype=None, out_nstride=0, out_hw=None, splitk_ws=None,
           in_cstride=None, w_x3=None, _no_tape=False, stop_grad=False, bn_raw=False, in_pair=False, out_pair=False,
           w_h2=None, out2=None, out2_coff=0, res1_up=False, in_up2=False, nxt=None, nxt_out=None, nxt_out_coff=0):
    """Channel-last implicit-GEMM convolution on MFMA (tt_conv2d_fwd).

    x   [N,H,W,Cs]  (f32 or bf16); channels [in_coff, in_coff+cin) are convolved
    w   [Cout,KH,KW,cin] same dtype (for pixel_shuffle2: [4*Cout_real,1,1,cin])
    out [N,OH,OW,Ct] written at channel offset out_coff (allocated if None)
    res1_up: res1 is a coarser [N, h, w, C] map added through nearest upsampling to the output size (PAFPN top-down path)
    w_h2: (x, w half) the f16 (hi, lo) weight pair of weights.split_pairs_h2 -- the layer runs the two-MFMA "h2" product
    out2 / out2_coff: optional second, f32, copy of the output rows at channel offset out2_coff of a [.., Ct2] tensor
    in_pair / out_pair (bf16x3 layers only): x is / out becomes a PAIR-format tensor (an f32-typed container holding, per 16
    channels, the bf16 hi and lo halves the kernel's operand split would produce: tt_conv_desc.in_pair).  Only for tensors whose
    every reader is a bf16x3 convolution (`pair_ok` says whether a layer of those numbers takes one).
    in_up2 (bf16x3 3 x 3 / stride 1 / pad 1 layers with 64 output channels; `up2_ok` says which): x is the low-resolution f32 map
    [N, h, w, C] and the layer convolves bilinear_up2(x) -- nn.Upsample(scale_factor=2, bilinear, align_corners=True) -- without that
    tensor ever existing (tt_conv_desc.in_up2); bit for bit conv2d(bilinear_up2(x, out_pair=True), ..., in_pair=True).
    nxt (bf16x3 1 x 1 / stride 1 layers; `join_ok` says which): (w, w_x3, scale, shift, act) of the 1 x 1 convolution that reads this
    layer's output.  It runs in the SAME launch on each row tile of `out` while that is still on chip (tt_conv2d_fwd_next), and
    conv2d returns (out, next_out) with next_out [N, OH, OW, w.shape[0]] in PAIR format; both are bit for bit what the two conv2d
    calls give (a ResNet bottleneck's conv3 and the next block's conv1).  nxt_out / nxt_out_coff: the tensor (and channel offset)
    next_out is written into instead of a new one.  Inference only.
    The `*_ok` predicates (section "routes" below) are where the model chooses among these forms; they ask the library.
    in_cstride / out_hw: "row-run" form -- the kernel reads `cin` CONTIGUOUS elements starting at pixel (ih, iw) of a
    tensor whose pixels are only Cs < cin elements apart (a run of cin/Cs pixels along W), with the output size given
    explicitly; used for the 7x7/2 stem (lss.py).
    """
    require_cuda(x, w)
    assert w.is_contiguous() and x.dim() == 4 and w.dim() == 4
    N, H, W, Cs = x.shape
    # inner (H, W, C) block must be dense; the image (batch) stride may be anything
    xst = x.stride()
    assert xst[3] == 1 and (W == 1 or xst[2] == Cs) and (H == 1 or xst[1] == W * Cs), xst
    Cout, KH, KW, Cin = w.shape
    if cin is None:
        cin = Cin
    assert cin == Cin, (cin, Cin)
    if out is None:
        out_shape = conv_geometry(x.shape, w.shape, stride, pad, dil, out_hw, pixel_shuffle2, in_up2)[4]
        out = torch.empty(out_shape, dtype=out_dtype or x.dtype, device=x.device)
    x3, x3_splitk = _training_x3(w_x3, Cout, _in_training_step(_no_tape))
    # 1. the descriptor (a split-K query sees the bf16x3 operand only where a split-K launch would run with it)
    r1, r2, o2 = res1 is not None, res2 is not None, out2 is not None
    d = conv_desc(x.data_ptr(), x.shape, xst, w.data_ptr(), w.shape, out.data_ptr(), out.shape, out.stride(), dtype_code(x), dtype_code(out),
                  stride, pad, dil, out_hw, pixel_shuffle2, in_up2,
                  in_coff, in_cstride, out_coff, out_nstride,
                  ptr(scale), ptr(shift), ptr(shift_n), shift_n_mod, act,
                  ptr(res1), r1 and res1.shape, r1 and dtype_code(res1), res1_coff, res1_up, ptr(res2), r2 and res2.shape, res2_coff,
                  ptr(x3_splitk), ptr(w_h2), in_pair, out_pair, ptr(out2), o2 and out2.shape, out2_coff)
    OH, OW = d.OH, d.OW
    rows = N * OH * OW
    # 2. the operand modes: what each asks of the tensors, and the inference-only ones refused under a tape
    _refuse_on_tape(w_h2 is not None, in_pair or out_pair, in_up2, nxt is not None)
    if in_up2:
        assert x.dtype == torch.float32 and x.is_contiguous() and w_x3 is not None and not in_pair and splitk_ws is None
    if res1_up:
        assert res1 is not None and res1.dim() == 4 and res1.is_contiguous() and res1.shape[0] == N and splitk_ws is None
    if w_h2 is not None:
        assert x.dtype == torch.float16 and w.dtype == torch.float16 and w_h2.dtype == torch.float16 and w_h2.is_contiguous() \
            and w_h2.numel() == 2 * w.numel() and w_x3 is None and splitk_ws is None
    if out2 is not None:
        assert out2.dtype == torch.float32 and out2.numel() // out2.shape[-1] == rows and out2.stride(-1) == 1
    if in_pair or out_pair or nxt is not None:
        assert w_x3 is not None and x.dtype == torch.float32 and out.dtype == torch.float32 and splitk_ws is None
    if x3 is not None:
        assert x.dtype == torch.float32 and x3.shape == w.shape and x3.is_contiguous()
    # 3. the joined stage
    dn, nout = (None, None) if nxt is None else _joined_stage(nxt, nxt_out, nxt_out_coff, (N, OH, OW, Cout), x.device)
    # 4. the split-K workspace: the caller's, or one the library asks for; a launch without one runs with the bf16x3 operand
    if auto_splitk_asks(rows, KH * KW * Cin, splitk_ws is not None, in_pair or out_pair, in_up2, w_h2 is not None, res1_up):
        splitk_ws = _auto_splitk(d, x.device)
    if splitk_ws is not None:
        d.splitk_ws = splitk_ws.data_ptr()
    elif x3 is not None:
        d.weight_x3 = x3.data_ptr()
    # 5. the launch
    with _launch() as rec:
        if dn is not None:
            rc = lib().tt_conv2d_fwd_next(ctypes.byref(d), ctypes.byref(dn), _st(x))
        else:
            rc = lib().tt_conv2d_fwd(ctypes.byref(d), _st(x))
        check(rc, "tt_conv2d_fwd")
    if rec is not None:
        n2 = 0 if nout is None else nxt[0].shape[0]
        esz, osz = x.element_size(), out.element_size()
        in_px = min(N * H * W, rows * KH * KW)               # (source pixels) a strided 1x1 layer only touches the pixels it samples
        wsz = w.numel() * w.element_size() * (2 if w_h2 is not None else 1)
        rec.log(2.0 * rows * Cout * (KH * KW * Cin + n2),
                f"M={rows} N={Cout}->{n2} K={Cin} join k1x1s1" if n2 else f"M={rows} N={Cout} K={KH * KW * Cin} k{KH}x{KW}s{stride}",
                kernel=_last_conv_kernel,
                nbytes=(in_px * (in_cstride or Cin) * esz + rows * Cout * osz + wsz +
                        rows * Cout * esz * ((res1 is not None) + (res2 is not None)) +
                        (rows * Cout * 4 if out2 is not None else 0) +
                        (rows * n2 * 4 + nxt[0].numel() * 4 if n2 else 0)))     # a joined stage: its output and weights
    # 6. the tape
    if not _no_tape:
        _tape("conv", x, w, out, stride, pad, dil, scale, shift, act, in_coff, cin, out_coff, res1, res1_coff,
              res2, res2_coff, pixel_shuffle2, in_cstride, shift_n, shift_n_mod, stop_grad, bn_raw)
    return out if nout is None else (out, nout)


def seg_feedback_chain(x, cv1, cv2, out=None, out_coff=0):
    """Two 1 x 1 `layers.Conv` (folded BN, none / ReLU) over the pixels of x [N, H, W, Cs] in one launch (tt_seg_feedback_chain):
    cv1 Cs -> 64 on its plain f32 weights, cv2 64 -> 8 / 16 / 32 with its pair-format weights riding along.  Bit-equal to
    cv2(cv1(x)); the 64-channel map between them is never written.  Inference only (nothing is taped)."""
    require_cuda(x, cv1.w, cv2.w)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    assert cv2.w_x3 is not None and cv1.w.dtype == torch.float32 and cv2.w.dtype == torch.float32
    N, H, W, Cs = x.shape
    n1, kh1, kw1, k1 = cv1.w.shape
    n2, kh2, kw2, k2 = cv2.w.shape
    assert (kh1, kw1, kh2, kw2) == (1, 1, 1, 1) and k1 == Cs and k2 == n1 == 64, (cv1.w.shape, cv2.w.shape, Cs)
    assert (cv1.stride, cv1.pad, cv2.stride, cv2.pad) == (1, 0, 1, 0) and not cv1.ps2 and not cv2.ps2
    if out is None:
        out = torch.empty(N, H, W, n2, dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() // out.shape[-1] == N * H * W
    R = N * H * W
    with _launch() as rec:
        check(lib().tt_seg_feedback_chain(ptr(x), R, Cs, k1, ptr(cv1.w), ptr(cv1.scale), ptr(cv1.shift), cv1.act, ptr(cv2.w),
                                          ptr(cv2.w_x3), n2, ptr(cv2.scale), ptr(cv2.shift), cv2.act, ptr(out), out.shape[-1],
                                          out_coff, _st(x)), "tt_seg_feedback_chain")
    if rec is not None:
        rec.log(2.0 * R * (k1 * n1 + k2 * n2), f"M={R} N={n1}->{n2} K={k1} chain k1x1s1", kernel="seg_chain_kernel",
                nbytes=R * (Cs + n2) * 4 + (cv1.w.numel() + cv2.w.numel()) * 4)
    return out


# ----------------------------------------------------------------------------- train-mode BatchNorm / dropout
BN_SYNC = True          # SyncBN (configs/thinktwice.py:39): all-reduce the batch statistics when torch.distributed runs > 1 rank
DROPOUT_MASKS = None    # tests: iterator of host uint8 keep-masks (the reference's torch masks) consumed by dropout()
DROPOUT_SEED = [0x5EED, 0]    # [seed, calls so far]: the product's counter-based generator


def _all_reduce_sum_(t):
    """In-place SUM over the ranks (no-op on a single rank): the SyncBN statistic exchange."""
    import torch.distributed as dist
    if not (BN_SYNC and dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return t
    if t.is_cuda and dist.get_backend() == "gloo":        # CPU test rigs: stage through the host
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


class BNSpec:
    """One BatchNorm layer's tensors for the train-mode path (device f32): affine, running statistics (updated in place),
    eps / momentum, and the state_dict prefix the parameter gradients are filed under."""

    def __init__(self, name, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1):
        self.name, self.gamma, self.beta, self.running_mean, self.running_var = name, gamma, beta, running_mean, running_var
        self.eps, self.momentum = float(eps), float(momentum)


def batchnorm_train(z, spec, act=0, res1=None, res1_coff=0, res2=None, res2_coff=0, out=None, out_coff=0, m_dev=None,
                    groups=1, update_running=True):
    """y = act(BN_batch(z) + res1 + res2): z [..., C] dense f32 rows (the raw conv output, bias included); out: row-linear
    buffer [..., Ct] written at channel offset out_coff (allocated if None).  `groups` equal row groups get their own
    statistics; m_dev: device count of live rows (sparse levels).  SyncBN: one all-reduce of the statistics block."""
    require_cuda(z)
    assert z.dtype == torch.float32 and z.is_contiguous()
    C = z.shape[-1]
    M = z.numel() // C
    dev = z.device
    if out is None:
        out = torch.empty_like(z)
    assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() // out.shape[-1] == M, (out.shape, z.shape)
    for r in (res1, res2):
        assert r is None or (r.is_contiguous() and r.dtype == torch.float32 and r.numel() // r.shape[-1] == M)
    stats = torch.empty(groups, 2 * C + 2, dtype=torch.float64, device=dev)
    L = lib()
    ws = _workspace(L.tt_bn_workspace_bytes(C, groups), dev)
    nb, st = ws.numel(), _st(z)
    check(L.tt_bn_stats(ptr(z), M, C, C, 0, ptr(m_dev), groups, ptr(stats), ptr(ws), nb, st), "tt_bn_stats")
    _all_reduce_sum_(stats)
    scale, shift, mean, invstd = (torch.empty(groups, C, dtype=torch.float32, device=dev) for _ in range(4))
    check(L.tt_bn_finalize(ptr(stats), C, groups, ptr(spec.gamma), ptr(spec.beta), spec.eps, spec.momentum,
                           ptr(spec.running_mean if update_running else None),
                           ptr(spec.running_var if update_running else None), ptr(scale), ptr(shift), ptr(mean), ptr(invstd),
                           st), "tt_bn_finalize")
    check(L.tt_bn_apply(ptr(z), M, C, C, 0, ptr(m_dev), groups, ptr(scale), ptr(shift), ptr(mean), ptr(res1), _cs(res1),
                        res1_coff, ptr(res2), _cs(res2), res2_coff, act, ptr(out), out.shape[-1], out_coff, st), "tt_bn_apply")
    _tape("bn_train", z, out, out_coff, spec, act, res1, res1_coff, res2, res2_coff, m_dev, groups, stats, scale, mean, invstd)
    return out


def batchnorm_train_bwd(dy, dy_coff, y, y_coff, z, mean, invstd, scale, stats, act, dres1, dres1_coff, dres2, dres2_coff, dz,
                        m_dev=None, groups=1):
    """Backward of batchnorm_train: dy (the gradient buffer of `out`, its channel window is overwritten with g), -> dz
    written, dres* accumulated; returns (dgamma [C], dbeta [C]) from the LOCAL sums."""
    C = z.shape[-1]
    M = z.numel() // C
    dev = z.device
    sums = torch.empty(groups, 2 * C, dtype=torch.float64, device=dev)
    L = lib()
    ws = _workspace(L.tt_bn_workspace_bytes(C, groups), dev)
    nb, st = ws.numel(), _st(z)
    check(L.tt_bn_bwd_reduce(ptr(dy), dy.shape[-1], dy_coff, ptr(y), y.shape[-1], y_coff, ptr(z), C, 0,
                             M, C, ptr(m_dev), groups, ptr(mean), ptr(invstd), act, ptr(dres1), _cs(dres1),
                             dres1_coff, ptr(dres2), _cs(dres2), dres2_coff, ptr(sums), ptr(ws), nb, st), "tt_bn_bwd_reduce")
    local = sums.sum(0).to(torch.float32)
    _all_reduce_sum_(sums)
    check(L.tt_bn_bwd_apply(ptr(dy), dy.shape[-1], dy_coff, ptr(z), C, 0, M, C, ptr(m_dev), groups,
                            ptr(sums), ptr(stats), ptr(scale), ptr(mean), ptr(invstd), ptr(dz), dz.shape[-1], 0, st),
          "tt_bn_bwd_apply")
    return local[C:].contiguous(), local[:C].contiguous()


def dropout(x, p=0.5):
    """nn.Dropout(p) in train mode (lss.py:91,110).  Keep-mask from the counter-based device generator, or -- tests -- the next
    host mask of DROPOUT_MASKS (the reference's own torch mask, in x's channel-last layout)."""
    require_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty_like(x)
    mask = torch.empty(x.numel(), dtype=torch.uint8, device=x.device)
    mask_in = None
    if DROPOUT_MASKS is not None:
        mask_in = next(DROPOUT_MASKS).to(device=x.device, dtype=torch.uint8).contiguous()
        assert mask_in.numel() == x.numel()
    DROPOUT_SEED[1] += 1
    seed = (DROPOUT_SEED[0] * 0x100000001B3 + DROPOUT_SEED[1] * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    check(lib().tt_dropout_fwd(ptr(x), ptr(out), x.numel(), p, seed, ptr(mask_in), ptr(mask), _st(x)), "tt_dropout_fwd")
    _tape("dropout", x, out, mask, p)
    return out


def dropout_bwd(dout, mask, dx, p):
    assert dout.is_contiguous() and dx.is_contiguous()
    check(lib().tt_dropout_bwd(ptr(dout), ptr(mask), ptr(dx), dout.numel(), p, _st(dout)), "tt_dropout_bwd")


def nchw_to_nhwc_border(x, out, top, left):
    """(N,C,H,W) f32 -> interior of out (N,Hp,Wp,Cp) at pixel offset (top, left); border untouched."""
    require_cuda(x, out)
    assert x.is_contiguous() and x.dtype == torch.float32 and out.is_contiguous()
    N, C, H, W = x.shape
    _, Hp, Wp, Cp = out.shape
    check(lib().tt_nchw_to_nhwc_border(ptr(x), ptr(out), N, C, H, W, Cp, Hp, Wp,
                                       top, left, dtype_code(out), _st(x)), "tt_nchw_to_nhwc_border")
    return out


def nchw_to_nhwc_pad(x, dtype, c_pad):
    """(N,C,H,W) f32 -> (N,H,W,c_pad) `dtype`, zero-padded channels."""
    require_cuda(x)
    assert x.is_contiguous() and x.dtype == torch.float32
    N, C, H, W = x.shape
    out = torch.empty(N, H, W, c_pad, dtype=dtype, device=x.device)
    check(lib().tt_nchw_to_nhwc_pad(ptr(x), ptr(out), N, C, H, W, c_pad, dtype_code(out), _st(x)), "tt_nchw_to_nhwc_pad")
    return out


def nhwc_to_nchw(x, C=None, coff=0):
    """(N,H,W,Cs) -> (N,C,H,W) f32."""
    require_cuda(x)
    N, H, W, Cs = x.shape
    C = C or Cs
    out = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
    check(lib().tt_nhwc_to_nchw(ptr(x), ptr(out), N, C, H, W, Cs, coff, dtype_code(x), _st(x)), "tt_nhwc_to_nchw")
    return out


def maxpool3x3s2(x):
    N, H, W, C = x.shape
    out = torch.empty(N, (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1, C, dtype=x.dtype, device=x.device)
    check(lib().tt_maxpool3x3s2(ptr(x), ptr(out), N, H, W, C, dtype_code(x), _st(x)), "tt_maxpool3x3s2")
    _tape("maxpool3x3s2", x, out)
    return out


def stem_pool(img, w_x3, scale, shift, max_workgroups=0):
    """img (B, T, N, 3, H, W) f32 (any b / t / n strides) -> max_pool2d(relu(scale * conv7x7s2p3(img) + shift), 3, 2, 1) as f32
    (T*B*N, ceil(H/4), ceil(W/4), 64) channel-last, images sweep-major ((s*B + b)*N + n = img[b, T-1-s, n]).  w_x3: the row-run
    stem weights [64][7][1][32] in pair format.  Bit-equal to nchw_to_nhwc_border + conv2d(row-run) + maxpool3x3s2."""
    require_cuda(img, w_x3, scale, shift)
    B, T, N, C, H, W = img.shape
    NI, PH, PW = B * T * N, (H // 2 + 1) // 2, (W // 2 + 1) // 2
    out = torch.empty(NI, PH, PW, 64, dtype=torch.float32, device=img.device)
    sb, st, sn, sc, sh, sw = img.stride()
    with _launch() as rec:
        check(lib().tt_stem_pool_x3(ptr(img), sb, st, sn, sc, sh, sw, B, T, N, H, W, dtype_code(img), ptr(w_x3), w_x3.shape[0],
                                    w_x3.shape[1], w_x3.shape[-1], ptr(scale), ptr(shift), ptr(out), out.numel(), max_workgroups,
                                    _st(img)), "tt_stem_pool_x3")
    if rec is not None:
        M = NI * (H // 2) * (W // 2)
        rec.log(2.0 * M * 64 * 224, f"M={M} N=64 K=224 stem+pool k7x7s2", kernel="conv_x3_stem_pool_kernel",
                nbytes=NI * 3 * H * W * 4 + out.numel() * 4 + w_x3.numel() * 4)
    return out


def upsample_nearest_add_(dst, src):
    N, H, W, C = dst.shape
    check(lib().tt_upsample_nearest_add(ptr(dst), ptr(src), N, H, W, C, src.shape[1],
                                        src.shape[2], dtype_code(dst), _st(dst)), "tt_upsample_nearest_add")
    _tape("upsample_nearest_add_", dst, src)
    return dst


# ----------------------------------------------------------------------------- routes: which layer takes an inference-only form
# The model picks a tensor's form before the tensor exists, so it asks these predicates with plain numbers.  None restates a kernel's
# contract: the shape part of an answer is the library's (tt_conv2d_plan about the form's canonical layer), the row bound is the
# header's SMALL_ROWS, the rest is `inference` and the route's A/B knob (an env switch and test hook, read by its one predicate).
PAIR = os.environ.get("TT_X3_PAIR", "1") != "0"             # 0 = every activation tensor stays plain f32
BNECK_JOIN = os.environ.get("TT_BNECK_JOIN", "1") != "0"    # 0 = a bottleneck's conv3 and the next block's conv1 stay two launches
SEG_UP2 = os.environ.get("TT_SEG_UP2", "1") != "0"          # 0 = unet_layer0's upsample and its 3 x 3 conv stay two launches
STEM_POOL = os.environ.get("TT_STEM_POOL", "1") != "0"      # 0 = border copy, row-run stem and max pool stay three launches
SEG_CHAIN = os.environ.get("TT_SEG_CHAIN", "1") != "0"      # 0 = the two seg feedback convs stay two launches


def inference(*x3, dtype=None, bn_train=False):
    """The gate of every inference-only route: no active tape, eval-mode BatchNorm (bn_train=True: either mode), the bf16x3 operand
    on every layers.Conv (or bare weight_x3) in `x3`, f32 storage where the site names its activations' `dtype`."""
    from . import layers
    return (_active_tape() is None and (bn_train or not layers.BN_TRAIN) and dtype in (None, torch.float32) and
            all(getattr(c, "w_x3", c) is not None for c in x3))


def canonical_desc(form, rows, cin, cout, arg=0):
    """(tt_conv_desc, tt_conv_next or None) of a form's CANONICAL layer from plain numbers, every operand at one stand-in aligned
    address (the planner looks at null-ness and alignment only): bf16x3, one image of 1 x rows pixels, a dense cout-channel output.
    "pair": k x k / pad k // 2, arg = k * k taps, pair-format input; "up2": the 3 x 3 in_up2 layer over the 2 x rows / 2 map;
    "join": the 1 x 1 layer (pair-format input, folded BN, residual, ReLU) with the joined stage cout -> arg."""
    P, k, up2, n = 0x10000, {"pair": math.isqrt(arg), "up2": 3, "join": 1}[form], form == "up2", None
    x, o = (1, 1, rows // 4 if up2 else rows, cin), ((1, 2, rows // 2, cout) if up2 else (1, 1, rows, cout))
    epi = dict(scale=P, shift=P, act=1, res1=P, res1_shape=o) if form == "join" else {}
    d = conv_desc(P, x, (0, 0, cin, 1), P, (cout, k, k, cin), P, o, (0, 0, cout, 1), TT_F32, TT_F32, pad=k // 2, weight_x3=P,
                  in_up2=up2, in_pair=not up2, **epi)
    if form == "join":
        n = _ConvNext()
        n.next_weight = n.next_weight_x3 = n.next_scale = n.next_shift = n.next_out = P
        n.next_cout = n.next_out_cstride = arg; n.next_act = n.next_out_pair = 1
    return d, n


def plan_label(d, nxt=None):
    """What tt_conv_last_kernel would report after launching `d` (with the joined stage `nxt`), or "ERROR: " + the refusal.  Host only."""
    L, buf = lib(), ctypes.create_string_buffer(192)
    rc = L.tt_conv2d_plan(ctypes.byref(d), buf, len(buf)) if nxt is None else \
        L.tt_conv2d_plan_next(ctypes.byref(d), ctypes.byref(nxt), buf, len(buf))
    return buf.value.decode() if rc == 0 else "ERROR: " + L.tt_last_error().decode()


@functools.lru_cache(maxsize=None)
def _taken(form, rows, cin, cout, arg=0):
    """Whether the library takes the form's canonical layer, and not below a routing threshold of its own (conv_choose.h,
    kJoinMinRows).  Asked once per set of numbers (no stream goes in, so a launch plan records none of this)."""
    label = plan_label(*canonical_desc(form, rows, cin, cout, arg))
    return not (label.startswith("ERROR") or label.endswith(" below kJoinMinRows"))


def pair_ok(rows, cin=32, cout=64, taps=9, x3=(), **gate):
    """Whether the input of the bf16x3 convolution with these numbers -- output rows, channels, KH * KW taps: the CONSUMER's, also
    when the tensor's producer asks -- is in pair format (tt_conv_desc.in_pair).  `x3`, `gate`: see inference."""
    return PAIR and inference(*x3, **gate) and rows > SMALL_ROWS and _taken("pair", rows, cin, cout, taps)


def up2_ok(rows, cin, cout, x3=(), **gate):
    """Whether the 3 x 3 bf16x3 convolution with this many OUTPUT rows reads its input through the bilinear x2 upsampling (in_up2)."""
    return SEG_UP2 and inference(*x3, **gate) and rows > SMALL_ROWS and _taken("up2", rows, cin, cout)


# the (Cin, Cout, next Cout) forms of the joined kernel that beat their two launches at the model's row counts
# (profiles/bottleneck_join.txt); the library also takes (128, 512, 256) and (256, 1024, 256), which lose there
JOIN_ROUTED = ((64, 256, 64), (64, 256, 128), (128, 512, 128))


def join_ok(rows, k1, cout, next_cout, x3=()):
    """Whether the 1 x 1 bf16x3 convolution k1 -> cout over these rows also runs the next 1 x 1 layer, cout -> next_cout (nxt=...)."""
    return BNECK_JOIN and inference(*x3) and (k1, cout, next_cout) in JOIN_ROUTED and _taken("join", rows, k1, cout, next_cout)


def res1_up_ok(rows, dtype=torch.float32):
    """Whether a conv over these rows adds a coarser map through nearest upsampling in its epilogue (res1_up; PAFPN top-down path)."""
    return inference(dtype=dtype) and rows > SMALL_ROWS


def seg_chain_ok(cv2, dtype):
    """Whether the two seg feedback convs run as one launch (seg_feedback_chain); cv2: the second of them."""
    return SEG_CHAIN and inference(cv2, dtype=dtype)


def stem_pool_ok(img, w_x3):
    """Whether the bf16x3 stem runs from the NCHW image to the pooled map in one launch (stem_pool): even H and W, a contiguous
    (3, H, W) block per image, and more than SMALL_ROWS stem pixels: up to there the three launches run the latency kernel."""
    if not (STEM_POOL and inference(w_x3, dtype=img.dtype) and img.dim() == 6 and img.shape[3] == 3 and img.shape[4] % 2 == 0 and
            img.shape[5] % 2 == 0):
        return False
    B, T, N, _, H, W = img.shape
    return tuple(img.stride()[3:]) == (H * W, W, 1) and B * T * N * (H // 2) * (W // 2) > SMALL_ROWS


def bilinear_up2(x, out_pair=False):
    N, H, W, C = x.shape
    out = torch.empty(N, 2 * H, 2 * W, C, dtype=x.dtype, device=x.device)
    if out_pair:      # f32 -> bf16x3 pair format for a consumer that is a bf16x3 convolution (conv2d(in_pair=True))
        assert x.dtype == torch.float32 and x.is_contiguous() and C % 16 == 0
        check(lib().tt_bilinear_up2_pair(ptr(x), ptr(out), N, H, W, C, _st(x)), "tt_bilinear_up2_pair")
        return out
    check(lib().tt_bilinear_up2(ptr(x), ptr(out), N, H, W, C, dtype_code(x), _st(x)), "tt_bilinear_up2")
    _tape("bilinear_up2", x, out)
    return out


def spatial_pool(x, mode, C=None, coff=0):
    """(N,H,W,Cs) -> f32 (N,C): mode 0 mean, mode 1 (mean+max)/2."""
    N, H, W, Cs = x.shape
    C = C or Cs
    out = torch.empty(N, C, dtype=torch.float32, device=x.device)
    check(lib().tt_spatial_pool(ptr(x), ptr(out), N, H * W, C, Cs, coff, mode, dtype_code(x), _st(x)), "tt_spatial_pool")
    _tape("spatial_pool", x, out, mode, C, coff)
    return out


def channel_gate(x, gate, res=None, gate_act=_lib.ACT_SIGMOID, out_act=_lib.ACT_NONE, out=None):
    N, H, W, C = x.shape
    assert gate.dtype == torch.float32 and gate.shape == (N, C) and gate.is_contiguous()
    out = torch.empty_like(x) if out is None else out
    check(lib().tt_channel_gate(ptr(x), ptr(gate), ptr(res), ptr(out), N, H * W, C, gate_act,
                                out_act, dtype_code(x), _st(x)), "tt_channel_gate")
    _tape("channel_gate", x, gate, res, out, gate_act, out_act)
    return out


def affine_rows(x, scale, shift, act=0, out=None):
    """x (R, C) possibly a row-strided 2-D view."""
    R, C = x.shape
    out = torch.empty(R, C, dtype=x.dtype, device=x.device) if out is None else out
    check(lib().tt_affine_rows(ptr(x), ptr(scale), ptr(shift), ptr(out), R, C, x.stride(0),
                               out.stride(0), act, dtype_code(x), _st(x)), "tt_affine_rows")
    _tape("affine_rows", x, scale, shift, act, out)
    return out


def layernorm_rows(x, gamma, beta, eps=1e-5, out=None, D=None):
    """LayerNorm over the first D columns of each row of the 2-D (row-strided) x."""
    R = x.shape[0]
    D = D or x.shape[1]
    out = torch.zeros(R, x.shape[1], dtype=x.dtype, device=x.device) if out is None else out
    check(lib().tt_layernorm_rows(ptr(x), ptr(gamma), ptr(beta), ptr(out), R, D, x.stride(0),
                                  out.stride(0), eps, dtype_code(x), _st(x)), "tt_layernorm_rows")
    _tape("layernorm_rows", x, gamma, beta, out, D, eps)
    return out


def layernorm_rows_bwd(x, gamma, dout, dx, dgamma, dbeta, D, eps=1e-5):
    """dx[:, :D] += , dgamma += , dbeta += backward of layernorm_rows (2-D row-strided f32 views)."""
    R = x.shape[0]
    L = lib()
    ws = _workspace(L.tt_layernorm_rows_bwd_workspace_bytes(R, D), x.device)
    check(L.tt_layernorm_rows_bwd(ptr(x), ptr(gamma), ptr(dout), ptr(dx), ptr(dgamma), ptr(dbeta), R, D,
                                  x.stride(0), dout.stride(0), dx.stride(0), eps, ptr(ws), ws.numel(), _st(x)), "tt_layernorm_rows_bwd")


def concat_piece_bwd(dout, coff, C, div, mod, dsrc):
    """dsrc[:, :C] += the gradient of one concat_rows piece (dout / dsrc 2-D row-strided f32 views)."""
    R = dout.shape[0]
    check(lib().tt_concat_piece_bwd(ptr(dout), dout.stride(0), coff, R, C, div, mod, ptr(dsrc),
                                    dsrc.stride(0), dsrc.shape[0], _st(dout)), "tt_concat_piece_bwd")


def copy_nhwc(x, out, C=None, in_coff=0, out_coff=0, rot_flip=False):
    N, H, W, Cs = x.shape
    C = C or Cs
    check(lib().tt_copy_nhwc(ptr(x), ptr(out), N, H, W, C, Cs, in_coff, out.shape[-1], out_coff, 1 if rot_flip else 0,
                             dtype_code(x), dtype_code(out), _st(x)), "tt_copy_nhwc")
    _tape("copy_nhwc", x, out, C, in_coff, out_coff, rot_flip)
    return out


def broadcast_rows(v, out, out_coff=0):
    """v (N, C) -> out (N,H,W,Ct)[..., out_coff:out_coff+C] = v[n, :]."""
    N, C = v.shape
    _, H, W, Ct = out.shape
    check(lib().tt_broadcast_rows(ptr(v), ptr(out), N, H * W, C, v.stride(0), Ct,
                                  out_coff, dtype_code(out), _st(out)), "tt_broadcast_rows")
    _tape("broadcast_rows", v, out, out_coff)
    return out


def ew(op, a, b=None, g=None, out=None, C=None, a_coff=0, b_coff=0, g_coff=0, out_coff=0, act=0):
    """Row-wise elementwise op on 2-D (row-strided) views; see tt_ew."""
    a2 = a.reshape(-1, a.shape[-1])
    R = a2.shape[0]
    C = C or a2.shape[1]
    if out is None:
        out = torch.empty(R, C, dtype=a.dtype, device=a.device)
    o2 = out.reshape(-1, out.shape[-1])
    assert o2.data_ptr() == out.data_ptr() and o2.stride(1) == 1, "ew: `out` must be viewable as rows"
    b2 = None if b is None else b.reshape(-1, b.shape[-1])
    g2 = None if g is None else g.reshape(-1, g.shape[-1])
    check(lib().tt_ew(ptr(a2), ptr(b2), ptr(g2), ptr(o2), R, C, a2.stride(0), a_coff,
                      0 if b2 is None else b2.stride(0), b_coff, 0 if g2 is None else g2.stride(0),
                      g_coff, o2.stride(0), out_coff, op, act, dtype_code(a), _st(a)), "tt_ew")
    _tape("ew", op, act, R, C, a2, a_coff, b2, b_coff, g2, g_coff, o2, out_coff)
    return out


def ew_bwd(op, act, R, C, a2, a_coff, b2, b_coff, g2, g_coff, o2, out_coff, dout, da, db, dg):
    """Backward of `ew` on the same 2-D row views (d* are the gradient views of a2 / b2 / g2 / o2, or None)."""
    def st(t):
        return 0 if t is None else t.stride(0)
    check(lib().tt_ew_bwd(op, act, R, C, ptr(a2), st(a2), a_coff, ptr(b2), st(b2), b_coff, ptr(g2), st(g2), g_coff, ptr(o2),
                          st(o2), out_coff, ptr(dout), st(dout), out_coff, ptr(da), st(da), a_coff, ptr(db), st(db), b_coff,
                          ptr(dg), st(dg), g_coff, _st(a2)), "tt_ew_bwd")


def concat_rows(out, pieces, coff=0):
    """out (R, Ct) f32; pieces = [(src or None, C, div, mod), ...] laid out left to right from column `coff`:
    out[r, ...] = src[(r // div) % mod if mod else r // div, :C]  (None: zeros).  One launch (tt_concat_rows)."""
    o2 = out.reshape(-1, out.shape[-1])
    assert o2.data_ptr() == out.data_ptr() and o2.dtype == torch.float32 and 1 <= len(pieces) <= 8
    assert o2.stride(1) == 1, "concat_rows: `out` rows must be element-contiguous"
    n = len(pieces)
    srcs = (ctypes.c_void_p * n)()
    strides, widths, coffs, divs, mods = ((ctypes.c_int * n)() for _ in range(5))
    c = coff
    for i, (src, C, div, mod) in enumerate(pieces):
        if src is not None:
            s2 = src.reshape(-1, src.shape[-1])
            assert s2.dtype == torch.float32 and s2.stride(1) == 1 and s2.shape[1] >= C
            need = mod if mod else -(-o2.shape[0] // div)          # source rows the mapping reaches
            assert s2.shape[0] >= need, f"concat_rows: piece {i} has {s2.shape[0]} rows, mapping reads {need}"
            srcs[i], strides[i] = s2.data_ptr(), s2.stride(0)
        else:
            srcs[i], strides[i] = None, 0
        widths[i], coffs[i], divs[i], mods[i] = C, c, div, mod
        c += C
    check(lib().tt_concat_rows(ptr(o2), o2.shape[0], o2.stride(0), n, srcs, strides, widths, coffs, divs,
                               mods, _st(out)), "tt_concat_rows")
    _tape("concat_rows", o2, pieces, coff)
    return out


def deform_im2col3x3(x, offsets, pad=1):
    """x (N,H,W,C), offsets f32 (N,H,W,>=18) -> cols (N*H*W, 1, 9, C) (a [M,1,9,C] "image" for conv2d)."""
    N, H, W, C = x.shape
    assert offsets.dtype == torch.float32 and offsets.is_contiguous()
    cols = torch.empty(N * H * W, 1, 9, C, dtype=x.dtype, device=x.device)
    check(lib().tt_deform_im2col3x3(ptr(x), ptr(offsets), ptr(cols), N, H, W, C,
                                    offsets.shape[-1], pad, dtype_code(x), _st(x)), "tt_deform_im2col3x3")
    _tape("deform_im2col3x3", x, offsets, cols, pad)
    return cols


def repeat_rows(t, times):
    """t (R, C) -> (times * R, C), the rows repeated block-wise (torch's t.repeat(times, 1)); a copy the training tape
    knows how to differentiate (the gradient is the sum over the repeats)."""
    assert t.dim() == 2 and t.is_contiguous()
    out = torch.empty(times * t.shape[0], t.shape[1], dtype=t.dtype, device=t.device)
    nb = t.numel() * t.element_size()
    for k in range(times):          # `times` contiguous block copies (tt_copy_bytes): no torch kernel in the forward
        check(lib().tt_copy_bytes(out.data_ptr() + k * nb, ptr(t), nb, _st(t)), "tt_copy_bytes")
    _tape("repeat_rows", t, out, times)
    return out


# ----------------------------------------------------------------------------- look module
def look_project_pack(wp, lidar2img, ida_mat, img_hw):
    B = wp.shape[0]
    dev = wp.device
    ref = torch.empty(B, 4, 120, 2, dtype=torch.float32, device=dev)
    qos = torch.empty(B, 4, 120, dtype=torch.int32, device=dev)
    count = torch.empty(B, 4, dtype=torch.int32, device=dev)
    max_len = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib().tt_look_project_pack(B, ptr(wp), ptr(lidar2img), ptr(ida_mat), img_hw[0], img_hw[1],
                                     ptr(ref), ptr(qos), ptr(count), ptr(max_len), _st(wp)), "tt_look_project_pack")
    return ref, qos, count, max_len


def _level_args(maps):
    arr = (ctypes.c_void_p * 4)(*[m.data_ptr() for m in maps])
    return arr, _level_hw((m.shape[1], m.shape[2]) for m in maps)


def look_gather_query(qos, ref, wp, ctrl_sp, temporal, static, meas, flat, maps, row_stride=1544):
    B = wp.shape[0]
    out = torch.empty(B * 4 * 120, row_stride, dtype=torch.float32, device=wp.device)
    arr, hw = _level_args(maps)
    check(lib().tt_look_gather_query(B, ptr(qos), ptr(ref), ptr(wp), ptr(ctrl_sp), ptr(temporal), ptr(static),
                                     ptr(meas), ptr(flat), arr, hw, dtype_code(maps[0]), ptr(out),
                                     row_stride, _st(wp)), "tt_look_gather_query")
    _tape("look_gather_query", qos, ref, out, temporal, static, meas, flat, maps, row_stride)
    return out


def look_gather_query_bwd(B, qos, ref, dout, row_stride, dtemporal, dstatic, dmeas, dflat, dmaps):
    arr, hw = _level_args(dmaps)
    check(lib().tt_look_gather_query_bwd(B, ptr(qos), ptr(ref), ptr(dout), row_stride, ptr(dtemporal), ptr(dstatic),
                                         ptr(dmeas), ptr(dflat), arr, hw, _st(dout)), "tt_look_gather_query_bwd")


def msda_sample_bwd(B, value, coff, offsets, logits, ref, level_hw, dout, dvalue, doffsets, dlogits):
    hw = _level_hw(level_hw)
    assert value.dtype == torch.float32
    check(lib().tt_msda_sample_bwd(B, ptr(value), value.shape[-1], coff, ptr(offsets), ptr(logits), ptr(ref), hw,
                                   ptr(dout), ptr(dvalue), ptr(doffsets), ptr(dlogits), _st(dout)), "tt_msda_sample_bwd")


def sca_reduce_bwd(B, dout, max_len, dx):
    check(lib().tt_sca_reduce_bwd(B, ptr(dout), ptr(max_len), ptr(dx), _st(dout)), "tt_sca_reduce_bwd")


def msda_sample(value, offsets, logits, ref, level_hw, B, coff=0):
    """value (B*4, S, Cv) with Cv >= 256: samples channels [coff, coff+256)."""
    out = torch.empty(B * 4 * 120, 256, dtype=torch.float32, device=value.device)
    hw = _level_hw(level_hw)
    check(lib().tt_msda_sample_strided(B, ptr(value), dtype_code(value), value.shape[-1], coff,
                                       ptr(offsets), ptr(logits), ptr(ref), hw, ptr(out), _st(value)), "tt_msda_sample_strided")
    _tape("msda_sample", value, offsets, logits, ref, level_hw, B, coff, out)
    return out


def sca_reduce(x, max_len, B):
    out = torch.empty(B, 1024, dtype=torch.float32, device=x.device)
    check(lib().tt_sca_reduce(B, ptr(x), ptr(max_len), ptr(out), _st(x)), "tt_sca_reduce")
    _tape("sca_reduce", x, max_len, B, out)
    return out


# ----------------------------------------------------------------------------- decoder row chains (tt_mlp_chain)
_ChainStage = _lib.structs()["tt_chain_stage"]
_ChainChoice = _lib.structs()["tt_chain_choice"]


class ChainLinear:
    """One nn.Linear prepared for tt_mlp_chain: weight [N, K] (+ optional leading `side_k` columns that multiply a
    separate few-column input, e.g. cat([wp, h]) @ W^T = W[:, :2] wp + W[:, 2:] h) -> pair-format bf16x3 operand."""

    def __init__(self, w, bias, act=0, side_k=0, device="cuda"):
        from . import weights
        w = w.detach().to(device=device, dtype=torch.float32)
        self.side_k = side_k
        self.side_w = w[:, :side_k].contiguous() if side_k else None
        w = w[:, side_k:]
        self.N, self.K = w.shape
        assert self.K % 4 == 0, "ChainLinear: K must be a multiple of 4"
        self.Kp = (self.K + 15) // 16 * 16
        wp = torch.zeros((self.N + 31) // 32 * 32, self.Kp, dtype=torch.float32, device=device)
        wp[: self.N, : self.K] = w
        self.w = weights.split_pairs_frag(wp)
        self.bias = None if bias is None else bias.detach().to(device=device, dtype=torch.float32).contiguous()
        self.act = act


_chain_form = {}


def chain_is_wide(R):
    """Whether mlp_chain runs R rows on tt_mlp_chain_wide on the current device (callers order their stages for the form that
    runs): the form depends on the rows alone, so the library is asked, once, about the smallest chain there is."""
    key = (R, torch.cuda.current_device())
    if key not in _chain_form:
        one = (_ChainStage * 1)()
        one[0].w, one[0].K, one[0].Kp, one[0].N, one[0].in_sel = 16, 16, 16, 1, -1
        _chain_form[key] = bool(_chain_plan(R, 16, one, 1, None, None, torch.device("cuda", key[1])).wide)
    return _chain_form[key]


def chain_faults():
    """Blocking (device synchronise): non-zero if a tt_mlp_chain_wide launch on the current device gave up waiting at its
    barrier since the last `clear_device_faults()` (tests assert 0)."""
    return int(lib().tt_mlp_chain_wide_faults())


_wide_cap = {}


def chain_wide_max_workgroups(device):
    """Workgroups one tt_mlp_chain_wide launch may use on `device` (co-resident capacity / 2 concurrent launches)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _wide_cap:
        with torch.cuda.device(idx):
            cap = int(lib().tt_mlp_chain_wide_max_workgroups())
        if cap < 0:
            raise TTError(f"tt_mlp_chain_wide_max_workgroups failed: {lib().tt_last_error().decode()}")
        _wide_cap[idx] = cap
    return _wide_cap[idx]


def _chain_plan(R, x_stride, arr, n_split, groups, wide, device):
    """tt_mlp_chain_plan: the library's choice (csrc/chain_choose.cpp) for these rows, stages and hints on `device`."""
    c = _ChainChoice()
    check(lib().tt_mlp_chain_plan(R, x_stride, len(arr), arr, n_split, 0 if groups is None else max(1, groups),
                                  0 if wide is None else 2 if wide else 1, chain_wide_max_workgroups(device), ctypes.byref(c)),
          "tt_mlp_chain_plan")
    return c


def mlp_chain(x, stages, n_split=1, groups=None, wide=None):
    """x (R, >= K0) f32 rows (row-strided ok).  stages: list of dicts {lin: ChainLinear, src: -1 | earlier stage index,
    res: (tensor (R, *), coff) | None, side: tensor (R, >= side_k) | None, out: (tensor (R, *), coff) | None}.
    The library chooses the form (tt_mlp_chain_plan): few rows (<= 512) run tt_mlp_chain_wide, the columns of every stage over
    `groups` workgroups per row group (default: the widest stage's 32-column blocks, at most 16; capped so that all workgroups are
    co-resident); otherwise tt_mlp_chain (`n_split`: the single-stage column split of that kernel).  `wide`: force one form."""
    require_cuda(x)
    assert x.dim() == 2 and x.dtype == torch.float32 and x.stride(1) == 1
    R = x.shape[0]
    n = len(stages)
    arr = (_ChainStage * n)()
    for i, st in enumerate(stages):
        lin = st["lin"]
        d = arr[i]
        d.w = lin.w.data_ptr(); d.bias = ptr(lin.bias)
        d.K, d.Kp, d.N, d.act, d.in_sel = lin.K, lin.Kp, lin.N, lin.act, st.get("src", i - 1)
        res = st.get("res")
        if res is not None:
            t, coff = res
            assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= R and t.shape[1] >= coff + lin.N
            d.res, d.res_stride, d.res_coff = t.data_ptr(), t.stride(0), coff
        side = st.get("side")
        if lin.side_k:
            assert side is not None and side.dtype == torch.float32 and side.dim() == 2 and side.stride(1) == 1
            assert side.shape[0] >= R and side.shape[1] >= lin.side_k
            d.side, d.side_w, d.side_stride, d.side_k = side.data_ptr(), lin.side_w.data_ptr(), side.stride(0), lin.side_k
        out = st.get("out")
        if out is not None:
            t, coff = out
            assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= R and t.shape[1] >= coff + lin.N
            d.out, d.out_stride, d.out_coff = t.data_ptr(), t.stride(0), coff
    c = _chain_plan(R, x.stride(0), arr, n_split, groups, wide, x.device)
    if c.wide:
        ws = _workspace(c.workspace_bytes, x.device)
        rc = lib().tt_mlp_chain_wide(ptr(x), R, x.stride(0), n, arr, c.n_groups, ptr(ws), ws.numel(), _st(x))
        if rc != -4 or wide:
            check(rc, "tt_mlp_chain_wide")
            return
        # -4: the ticket slots of graph-captured launches are used up (a process that re-captures over and over): the
        # one-workgroup-per-row-block chain computes the same stages without a cross-workgroup barrier
    check(lib().tt_mlp_chain(ptr(x), R, x.stride(0), n, arr, n_split, _st(x)), "tt_mlp_chain")


# ----------------------------------------------------------------------------- convolution backward (training step)
def conv2d_wgrad(x, dy, kh, kw, stride=1, pad=0, dil=1, cin=None, in_coff=0, cout=None, dy_coff=0, cin_pad=None,
                 out=None, accumulate=False, x3=False):
    """Weight gradient of `conv2d` (tt_conv2d_wgrad): x [N,H,W,Cs] f32, dy [N,OH,OW,Cd] f32 (the gradient w.r.t. the
    convolution's raw output) -> dw [cout][kh][kw][cin_pad] f32 in the weight layout (added to `out` if accumulate)."""
    require_cuda(x, dy)
    assert x.dtype == torch.float32 and dy.dtype == torch.float32 and x.is_contiguous() and dy.is_contiguous()
    N, H, W, Cs = x.shape
    N2, OH, OW, Cd = dy.shape
    assert N2 == N
    cin = cin or (Cs - in_coff)
    cout = cout or (Cd - dy_coff)
    cin_pad = cin_pad or cin
    if out is None:
        assert not accumulate
        out = torch.empty(cout, kh, kw, cin_pad, dtype=torch.float32, device=x.device)
    assert tuple(out.shape) == (cout, kh, kw, cin_pad) and out.is_contiguous()
    L = lib()
    ws = _workspace(L.tt_conv2d_wgrad_workspace_bytes(N, OH, cout, cin, cin_pad, kh, kw), x.device)
    nb = ws.numel()
    name = "tt_conv2d_wgrad_x3" if x3 else "tt_conv2d_wgrad"   # x3: the forward's bf16x3 arithmetic (csrc/wgrad_choose.cpp: which layers)
    with _launch() as rec:
        check(getattr(L, name)(ptr(x), N, H, W, cin, Cs, in_coff, ptr(dy), OH, OW, cout, Cd, dy_coff, kh, kw, stride, pad, dil,
                               cin_pad, 1 if accumulate else 0, ptr(out), ptr(ws), nb, _st(x)), name)
    if rec is not None:
        def plan_label():
            label = ctypes.create_string_buffer(192)
            check(L.tt_conv2d_wgrad_plan(ptr(x), N, H, W, cin, Cs, in_coff, ptr(dy), OH, OW, cout, Cd, dy_coff, kh, kw, stride, pad,
                                         dil, cin_pad, 1 if accumulate else 0, ptr(out), ptr(ws), nb, int(x3), label, len(label)),
                  "tt_conv2d_wgrad_plan")
            return label.value.decode()
        rec.log(2.0 * N * OH * OW * cout * kh * kw * cin, f"wgrad M={N * OH * OW} N={cout} K={kh * kw * cin} k{kh}x{kw}s{stride}",
                kernel=plan_label, nbytes=(x.numel() + dy.numel() + out.numel()) * 4)
    return out


def dgrad_weight(w):
    """[Cout][KH][KW][Cin] -> [Cin][KH][KW][Cout] rotated by 180 degrees: the weights whose forward convolution over dy is
    the input gradient (layout plumbing; re-derived whenever the weights change)."""
    return w.flip(1, 2).permute(3, 1, 2, 0).contiguous()


def conv2d_dgrad(dy, w, in_hw, stride=1, pad=0, dil=1, x3=True, out=None, out_coff=0):
    """Input gradient of `conv2d`: dy [N,OH,OW,Cout] f32, w [Cout][KH][KW][Cin] f32 -> dx [N,H,W,Cin] f32.
    = tt_conv2d_fwd of dy (zero-inserted for stride > 1) with dgrad_weight(w) and padding dil*(K-1) - pad; `x3` runs it
    in bf16x3 like the forward of the headline mode (else exact f32).  With `out` the result is ADDED to the channel
    window [out_coff, out_coff + Cin) of that gradient buffer (the conv's residual input is the buffer itself)."""
    from . import weights
    require_cuda(dy, w)
    assert dy.dtype == torch.float32 and w.dtype == torch.float32
    Cout, KH, KW, Cin = w.shape
    H, W = in_hw
    N, OH, OW, Cd = dy.shape
    assert Cd == Cout
    fh, fw = H + 2 * pad - dil * (KH - 1), W + 2 * pad - dil * (KW - 1)     # stride-1 output size of the forward conv
    if stride > 1:
        z = torch.zeros(N, fh, fw, Cout, dtype=torch.float32, device=dy.device)
        z[:, :(OH - 1) * stride + 1:stride, :(OW - 1) * stride + 1:stride] = dy
        dy = z
    else:
        assert (OH, OW) == (fh, fw), ((OH, OW), (fh, fw))
    wt = dgrad_weight(w)
    if Cout % 4:        # the convolution wants 16-byte channel vectors: zero channels on both operands
        cp = (Cout + 3) // 4 * 4
        dy = torch.nn.functional.pad(dy, (0, cp - Cout))
        wt = torch.nn.functional.pad(wt, (0, cp - Cout))
    pad_h, pad_w = dil * (KH - 1) - pad, dil * (KW - 1) - pad
    assert pad_h == pad_w and pad_h >= 0, "conv2d_dgrad: square kernels with pad <= dil*(K-1)"
    wx = weights.split_pairs_x3(wt) if (x3 and Cout % 32 == 0) else None
    if out is not None:
        return conv2d(dy, wt, stride=1, pad=pad_h, dil=dil, w_x3=wx, out=out, out_coff=out_coff, res1=out,
                      res1_coff=out_coff, _no_tape=True)
    return conv2d(dy, wt, stride=1, pad=pad_h, dil=dil, w_x3=wx, _no_tape=True)


def conv_epilogue_bwd(dy, y, scale=None, shift=None, act=0, res1=None, res2=None, want_dres=False, dscale=None, dshift=None,
                      accumulate=False, C=None, dy_coff=0, y_coff=0, res1_coff=0, res2_coff=0, dres1=None, dres1_coff=0,
                      dres2=None, dres2_coff=0, dres_accumulate=True, m_dev=None, pre=None, conv_raw=None):
    """Backward of conv2d's fused epilogue (tt_conv_epilogue_bwd): dy / y / res* [..., Cs] f32 channel-last views of the
    same M rows (row stride = last dim) -> (dconv [M, C] dense f32, dres, dscale [C], dshift [C]).  `dres1` / `dres2`:
    gradient buffers of the residual inputs, g is added to (or, dres_accumulate=False, written over) their channel
    windows; with want_dres a dense [M, C] copy of g is returned instead."""
    require_cuda(dy, y)
    C = C or (y.shape[-1] - y_coff)
    M = y.numel() // y.shape[-1]
    assert dy.numel() // dy.shape[-1] == M and dy.dtype == torch.float32 and y.dtype == torch.float32
    dev = y.device
    dconv = torch.empty(M, C, dtype=torch.float32, device=dev)
    dres = None
    if want_dres:
        assert dres1 is None
        dres = dres1 = torch.empty(M, C, dtype=torch.float32, device=dev)
        dres1_coff, dres_accumulate = 0, False
    if dscale is None:
        dscale = torch.empty(C, dtype=torch.float32, device=dev)
        dshift = torch.empty(C, dtype=torch.float32, device=dev)
        accumulate = False
    L = lib()
    ws = _workspace(L.tt_conv_epilogue_bwd_workspace_bytes(C), dev)
    check(L.tt_conv_epilogue_bwd(ptr(dy), dy.shape[-1], dy_coff, ptr(y), y.shape[-1], y_coff, ptr(res1), _cs(res1), res1_coff,
                                 ptr(res2), _cs(res2), res2_coff, ptr(scale), ptr(shift), M, C, act, ptr(dconv), C, 0,
                                 ptr(dres1), _cs(dres1), dres1_coff, ptr(dres2), _cs(dres2), dres2_coff,
                                 1 if dres_accumulate else 0, ptr(dscale if scale is not None else None), ptr(dshift),
                                 1 if accumulate else 0, ptr(m_dev), ptr(pre), ptr(conv_raw), ptr(ws), ws.numel(), _st(y)),
          "tt_conv_epilogue_bwd")
    return dconv, dres, (dscale if scale is not None else None), dshift


def maxpool3x3s2_bwd(x, dy, dx):
    """dx += backward of maxpool3x3s2 (x: the forward input, dy: gradient of the pooled map); all f32 channel-last."""
    require_cuda(x, dy, dx)
    N, H, W, C = x.shape
    assert x.is_contiguous() and dy.is_contiguous() and dx.is_contiguous() and dx.shape == x.shape
    check(lib().tt_maxpool3x3s2_bwd(ptr(x), ptr(dy), ptr(dx), N, H, W, C, _st(x)), "tt_maxpool3x3s2_bwd")
    return dx


def bilinear_up2_bwd(dy, dx):
    """dx += backward of bilinear_up2 (align_corners x2)."""
    require_cuda(dy, dx)
    N, H, W, C = dx.shape
    assert dy.is_contiguous() and dx.is_contiguous() and tuple(dy.shape) == (N, 2 * H, 2 * W, C)
    check(lib().tt_bilinear_up2_bwd(ptr(dy), ptr(dx), N, H, W, C, _st(dy)), "tt_bilinear_up2_bwd")
    return dx


def channel_gate_bwd(x, gate, dy, dx, dgate, out_relu=None, dres=None):
    """dx += g * sigmoid(gate), dgate += sigmoid'(gate) * sum_hw g * x, g = dy (or dy * [out_relu > 0], then dres += g);
    all f32, x / dy / dx [N,H,W,C] contiguous."""
    require_cuda(x, gate, dy, dx, dgate)
    N, H, W, C = x.shape
    assert x.is_contiguous() and dy.is_contiguous() and dx.is_contiguous() and gate.is_contiguous() and dgate.is_contiguous()
    check(lib().tt_channel_gate_bwd(ptr(x), ptr(gate), ptr(dy), ptr(dx), ptr(dgate), N, H * W, C,
                                    ptr(out_relu), ptr(dres), _st(x)), "tt_channel_gate_bwd")


def spatial_meanmax_bwd(x, dpool, dx):
    """dx += backward of spatial_pool(x, 1) (0.5 mean + 0.5 amax); x / dx [N,H,W,C] contiguous f32, dpool [N,C]."""
    require_cuda(x, dpool, dx)
    N, H, W, C = x.shape
    assert x.is_contiguous() and dx.is_contiguous() and dpool.is_contiguous()
    check(lib().tt_spatial_meanmax_bwd(ptr(x), ptr(dpool), ptr(dx), N, H * W, C, _st(x)), "tt_spatial_meanmax_bwd")


def spatial_mean_bwd(dpool, dx, C, coff=0):
    """dx[n, :, :, coff:coff+C] += dpool[n] / (H*W)."""
    require_cuda(dpool, dx)
    N, H, W, Cs = dx.shape
    assert dpool.is_contiguous() and dx.is_contiguous() and tuple(dpool.shape) == (N, C)
    check(lib().tt_spatial_mean_bwd(ptr(dpool), ptr(dx), N, H * W, C, Cs, coff, _st(dx)), "tt_spatial_mean_bwd")


def deform_im2col3x3_bwd(x, offsets, gcols, gx, goff, pad=1):
    """gx += , goff += backward of deform_im2col3x3 (f32; gx in a fixed order, no atomics)."""
    require_cuda(x, offsets, gcols, gx, goff)
    N, H, W, C = x.shape
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (x, offsets, gcols, gx, goff))
    check(lib().tt_deform_im2col3x3_bwd(ptr(x), ptr(offsets), ptr(gcols), ptr(gx), ptr(goff), N, H, W, C,
                                        offsets.shape[-1], pad, _st(x)), "tt_deform_im2col3x3_bwd")


def broadcast_rows_bwd(dout, dv, out_coff):
    """dv (N, C) (row-strided) += per-image sums of dout (N,H,W,Ct)[..., out_coff:out_coff+C]."""
    N, C = dv.shape
    _, H, W, Ct = dout.shape
    check(lib().tt_broadcast_rows_bwd(ptr(dout), ptr(dv), N, H * W, C, Ct, out_coff, dv.stride(0),
                                      _st(dout)), "tt_broadcast_rows_bwd")


def upsample_nearest_add_bwd(ddst, dsrc):
    """dsrc += sum of ddst over the pixels that sampled it (backward of upsample_nearest_add_ w.r.t. src)."""
    require_cuda(ddst, dsrc)
    N, H, W, C = ddst.shape
    _, h, w, _ = dsrc.shape
    assert ddst.is_contiguous() and dsrc.is_contiguous()
    check(lib().tt_upsample_nearest_add_bwd(ptr(ddst), ptr(dsrc), N, H, W, C, h, w, _st(ddst)), "tt_upsample_nearest_add_bwd")
    return dsrc


# ----------------------------------------------------------------------------- composite decoder kernels
def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def look_query_ln(qos, ref, wp, ctrl, raw_ctrl, temporal, static, meas, flat, maps, gamma, beta, row_stride=1552,
                  eps=1e-5):
    """look_gather_query + LayerNorm(1543) in one launch -> (B*4*120, row_stride) rows, zero padded."""
    B = wp.shape[0]
    assert flat.is_contiguous() and meas.is_contiguous() and wp.is_contiguous() and ctrl.is_contiguous()
    out = torch.empty(B * 4 * 120, row_stride, dtype=torch.float32, device=wp.device)
    arr, hw = _level_args(maps)
    check(lib().tt_look_query_ln(B, ptr(qos), ptr(ref), ptr(wp), ptr(ctrl), 1 if raw_ctrl else 0, ptr(temporal),
                                 ptr(static), ptr(meas), ptr(flat), arr, hw, dtype_code(maps[0]), ptr(gamma),
                                 ptr(beta), eps, ptr(out), row_stride, _st(wp)), "tt_look_query_ln")
    return out


def msda_sample_ln(value, offsets, logits, ref, level_hw, B, coff, gamma, beta, eps=1e-5, max_len=None):
    """msda_sample + LayerNorm(256): -> (raw rows, normalised rows), both (B*4*120, 256) f32.  `max_len` (device int from
    look_project_pack): the rows of slots >= max_len are skipped and left unwritten (sca_reduce_ln never reads them)."""
    R = B * 4 * 120
    out = torch.empty(R, 256, dtype=torch.float32, device=value.device)
    out_ln = torch.empty(R, 256, dtype=torch.float32, device=value.device)
    hw = _level_hw(level_hw)
    check(lib().tt_msda_sample_ln(B, ptr(value), dtype_code(value), value.shape[-1], coff, ptr(offsets),
                                  ptr(logits), ptr(ref), hw, ptr(gamma), ptr(beta), eps, ptr(out), ptr(out_ln),
                                  ptr(max_len), _st(value)), "tt_msda_sample_ln")
    return out, out_ln


def msda_sample_proj_ln(maps, offsets, logits, ref, B, wvT, bias, vshift, gamma, beta, eps=1e-5, max_len=None):
    """msda_sample_ln without a projected value tensor (tt_msda_sample_proj_ln): `maps` = the four fpn_linear maps (B*4, H_l, W_l,
    256) f32, wvT (256 in, 256 out) = value_proj.weight^T, bias (256), vshift (4 levels, 4 cameras, 256) -> (raw rows, normalised
    rows), both (B*4*120, 256) f32."""
    R = B * 4 * 120
    dev = offsets.device
    assert all(m.dtype == torch.float32 and m.is_contiguous() and m.shape[-1] == 256 for m in maps)
    assert tuple(wvT.shape) == (256, 256) and wvT.is_contiguous() and tuple(vshift.shape) == (4, 4, 256) and vshift.is_contiguous()
    out = torch.empty(R, 256, dtype=torch.float32, device=dev)
    out_ln = torch.empty(R, 256, dtype=torch.float32, device=dev)
    arr, hw = _level_args(maps)
    check(lib().tt_msda_sample_proj_ln(B, arr, hw, ptr(offsets), ptr(logits), ptr(ref), ptr(wvT), ptr(bias), ptr(vshift),
                                       ptr(gamma), ptr(beta), eps, ptr(out), ptr(out_ln), ptr(max_len), _st(offsets)),
          "tt_msda_sample_proj_ln")
    return out, out_ln


def sca_reduce_ln(x, max_len, B, gamma, beta, eps=1e-5):
    out = torch.empty(B, 1024, dtype=torch.float32, device=x.device)
    check(lib().tt_sca_reduce_ln(B, ptr(x), ptr(max_len), ptr(gamma), ptr(beta), eps, ptr(out), _st(x)), "tt_sca_reduce_ln")
    return out


def dec_merge_in(fflat, look, temporal, meas, gamma, beta, eps=1e-5):
    B = look.shape[0]
    assert fflat.is_contiguous() and look.is_contiguous() and meas.is_contiguous()
    out = torch.empty(B * 4, 1024, dtype=torch.float32, device=look.device)
    check(lib().tt_dec_merge_in(B, ptr(fflat), ptr(look), ptr(temporal), ptr(meas), ptr(gamma), ptr(beta), eps,
                                ptr(out), _st(look)), "tt_dec_merge_in")
    return out


def dec_gru(wts, inp6, state, fut):
    """wts: dict from decoder_fused.prep_gru; inp6 (B,4,6), state (B,441,32), fut (B,4,441,32) all f32 contiguous."""
    B = state.shape[0]
    assert inp6.is_contiguous() and state.is_contiguous() and fut.is_contiguous()
    L = lib()
    scratch = torch.empty(L.tt_dec_gru_scratch_floats(B), dtype=torch.float32, device=state.device)
    check(L.tt_dec_gru(B, ptr(inp6), ptr(state), ptr(fut), ptr(scratch), wts["w0"], wts["wx"], wts["b0"], wts["w2"], wts["b2"],
                       ptr(wts["wd0"]), ptr(wts["bd0"]), ptr(wts["wd2"]), ptr(wts["bd2"]), _st(state)), "tt_dec_gru")
    return fut


def dec_flatten(wts, maps, want_mids=False):
    """maps (N,441,32) f32 contiguous -> (N,256) [, mids (N, 100*64 + 16*128 + 4*256)]."""
    N = maps.shape[0]
    assert maps.is_contiguous() and maps.dtype == torch.float32
    out = torch.empty(N, 256, dtype=torch.float32, device=maps.device)
    mids = torch.empty(N, 100 * 64 + 16 * 128 + 4 * 256, dtype=torch.float32, device=maps.device) if want_mids else None
    L = lib()
    scratch = torch.empty(L.tt_dec_flatten_scratch_floats(N), dtype=torch.float32, device=maps.device)
    check(L.tt_dec_flatten(N, ptr(maps), ptr(out), ptr(mids), ptr(scratch), wts["w"], wts["b"], ptr(wts["bn_scale"]),
                               ptr(wts["bn_shift"]), _st(maps)), "tt_dec_flatten")
    return (out, mids) if want_mids else out


def dec_bev_update(wts, bev, G, out):
    """bev (B,441,32), G (B,1152) -> out (B,441,32) (all f32 contiguous)."""
    B = bev.shape[0]
    assert bev.is_contiguous() and G.is_contiguous() and out.is_contiguous()
    L = lib()
    scratch = torch.empty(L.tt_dec_bev_update_scratch_floats(B), dtype=torch.float32, device=bev.device)
    check(L.tt_dec_bev_update(B, ptr(bev), ptr(G), ptr(out), 441 * 32, None, 0, ptr(scratch), ptr(wts["w0"]),
                              ptr(wts["b0"]), wts["w2"], ptr(wts["b2"]), _st(bev)), "tt_dec_bev_update")
    return out


_seg = _lib.structs()["tt_grad_seg"]        # GradSegTable packs it as three int64, not through ctypes
if [(n, getattr(_seg, n).offset) for n, _ in _seg._fields_] + [ctypes.sizeof(_seg)] != [("src", 0), ("dst_off", 8), ("count", 16), 24]:
    raise TTError("include/thinktwice_hip.h: tt_grad_seg is no longer {src, dst_off, count} of 8 bytes each, as GradSegTable packs it")


class GradSegTable:
    """The segment table of tt_grad_gather for one device: `tt_grad_seg` records {src pointer, dst offset, count} (three 64-bit
    fields) written into a PINNED host buffer and uploaded to its device twin on the current stream.  The buffers grow as
    needed and are reused; an event guards the host buffer against being rewritten while the previous upload is in flight."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.host = self.dev = self.event = None
        self.nseg = self.flat_numel = 0

    def upload(self, srcs, dst_offs, flat_numel):
        """`srcs`: contiguous f32 device tensors (views are fine); `dst_offs`: their first element in the flat buffer.  The
        records are sorted by destination and checked on the host (inside `flat_numel`, no overlap): the kernel trusts them."""
        order = sorted(range(len(srcs)), key=lambda i: dst_offs[i])
        rec, end = [], 0
        for i in order:
            s, off = srcs[i], int(dst_offs[i])
            require_cuda(s)
            if s.dtype != torch.float32 or not s.is_contiguous() or s.device != self.device:
                raise TTError("grad_gather: sources are contiguous f32 tensors on the table's device")
            if off < end or off + s.numel() > flat_numel:
                raise TTError(f"grad_gather: segment [{off}, {off + s.numel()}) overlaps its neighbour or leaves the flat "
                              f"buffer of {flat_numel} elements")
            end = off + s.numel()
            rec += [s.data_ptr(), off, s.numel()]
        self.nseg, self.flat_numel = len(order), int(flat_numel)
        if self.nseg == 0:
            return self
        if self.host is None or self.host.numel() < len(rec):
            cap = max(len(rec), 3 * 1024)
            self.host = torch.empty(cap, dtype=torch.int64, pin_memory=True)
            self.dev = torch.empty(cap, dtype=torch.int64, device=self.device)
            self.event = torch.cuda.Event()
        else:
            self.event.synchronize()
        self.host[:len(rec)] = torch.tensor(rec, dtype=torch.int64)
        self.dev[:len(rec)].copy_(self.host[:len(rec)], non_blocking=True)
        self.event.record(torch.cuda.current_stream(self.device))
        return self


def grad_gather(table, flat, scale=None, accumulate=False):
    """flat[dst_off_i .. + count_i) (=|+=) scale * src_i for every segment of `table` (a GradSegTable uploaded on this
    stream), ONE launch; `scale`: device f32 scalar or None (1.0).  Elements no segment covers are not written.  The sources
    must stay allocated until the launch is issued (stream order does the rest)."""
    require_cuda(flat, scale)
    if flat.dtype != torch.float32 or not flat.is_contiguous() or flat.device != table.device or flat.numel() < table.flat_numel:
        raise TTError("grad_gather: the destination is a contiguous f32 buffer on the table's device, of the size the table "
                      "was checked against")
    if scale is not None and (scale.dtype != torch.float32 or scale.numel() != 1 or scale.device != flat.device):
        raise TTError("grad_gather: scale is one f32 value on the destination's device")
    check(lib().tt_grad_gather(ptr(table.dev), table.nseg, ptr(flat), ptr(scale), 1 if accumulate else 0, _st(flat)),
          "tt_grad_gather")
    return flat
