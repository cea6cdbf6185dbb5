/*
 * thinktwice_hip.h -- C ABI of libthinktwice_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the per-frame forward path of OpenDriveLab/ThinkTwice
 * (reference: open_loop_training/).  Every entry point takes raw DEVICE
 * pointers, plain sizes and a hipStream_t passed as void*; buffers are
 * caller-owned; calls are asynchronous on the given stream; return value is
 * 0 on success and <0 on error (tt_last_error() holds the text).  Nothing
 * here ever calls exit() (the reference launcher does: ops/voxel_pooling/src/
 * voxel_pooling_forward_cuda.cu:51-55).
 *
 * dtype codes: TT_F32 = 0 (exact f32 MFMA path, parity mode), TT_BF16 = 1
 * (bf16 storage, f32 accumulate).
 */
#ifndef THINKTWICE_HIP_H
#define THINKTWICE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TT_F32 0
#define TT_BF16 1
#define TT_F16 2   /* IEEE half storage, f32 accumulate (v_mfma_f32_32x32x16_f16): same rate as bf16, 8x finer rounding */

/* activation codes for fused epilogues */
#define TT_ACT_NONE 0
#define TT_ACT_RELU 1
#define TT_ACT_SIGMOID 2
#define TT_ACT_GELU 3
#define TT_ACT_SOFTPLUS 4
#define TT_ACT_SOFTPLUS_CLAMP 5  /* clamp(softplus(x), min=1e-3): thinktwice_decoder.py:484 */

const char* tt_last_error(void);
/* measurement aid: name (template arguments spelled like rocprofv3 prints them) of the kernel that the last
 * tt_conv2d_fwd call of this thread launched; "" before the first call */
const char* tt_conv_last_kernel(void);
/* measurement aid: while set, every workgroup of the LDS-DMA conv kernel writes 4 wall-clock stamps (10 ns ticks: entry, first K tile
 * landed, K loop done, epilogue done) at stamps[blockIdx.x * 4]; null (default) = off */
int tt_conv_set_trace(void* stamps_or_null);
int tt_version(void);

/* ------------------------------------------------------------------------
 * B1: voxel pooling (Lift-Splat "splat").
 * Replaces voxel_pooling_forward_wrapper
 *   (ops/voxel_pooling/src/voxel_pooling_forward.cpp:24-37) and its kernel
 *   (ops/voxel_pooling/src/voxel_pooling_forward_cuda.cu:9-36), argument for
 *   argument: geom_xyz int32 [B,Np,3]; input_features f32 [B,Np,C];
 *   output_features f32 [B,Y,X,C] caller-allocated and pre-zeroed; pos_memo
 *   int32 [B,Np,3] caller-allocated and pre-filled with -1 (may be NULL in
 *   inference -- the reference always writes it).
 * ---------------------------------------------------------------------- */
int tt_voxel_pool_fwd(int batch_size, int num_points, int num_channels,
                      int num_voxel_x, int num_voxel_y, int num_voxel_z,
                      const int32_t* geom_xyz, const float* input_features,
                      float* output_features, int32_t* pos_memo, void* stream);

/* Same operator with a caller-provided workspace.  Three arms, chosen per call in csrc/voxel_pool_choose.cpp:
 *   counting sort  the in-range points are sorted by (sample, cell) per launch (vp_cs_count / _scan / _scatter) and streamed by
 *                  the planned kernels: no atomics, deterministic, bit-identical to the static plan below.  From 32,768 points,
 *                  <= 1024 cells, <= 524,288 points per sample, C a multiple of 4 up to 1024; TT_VP_SORT=0 turns it off.
 *   two-phase      per-chunk cell sums in LDS order (voxel_pool_p1_kernel), then an ordered per-cell gather (_p2_kernel).  From
 *                  8,192 points, <= 2048 cells, the same C.
 *   atomic         tt_voxel_pool_fwd's single-pass kernels, when the workspace is missing or too small for the other two, a
 *                  buffer is not 16-byte aligned (the table in voxel_pool_choose.h), or the shape fits neither.
 * tt_voxel_pool_workspace_bytes is the most any arm takes for the sizes (0: only the atomic arm takes them). */
long long tt_voxel_pool_workspace_bytes(int batch_size, int num_points, int num_channels,
                                        int num_voxel_x, int num_voxel_y);
int tt_voxel_pool_fwd_ws(int batch_size, int num_points, int num_channels,
                         int num_voxel_x, int num_voxel_y, int num_voxel_z,
                         const int32_t* geom_xyz, const float* input_features,
                         float* output_features, int32_t* pos_memo,
                         void* workspace, long long workspace_bytes, void* stream);
/* Host only: which kernels tt_voxel_pool_fwd_ws (ws_entry != 0) / tt_voxel_pool_fwd (ws_entry = 0: the workspace is ignored) would
 * run these arguments on, assuming the device grants the counting sort its dynamic LDS.  Runs the validation and the dispatch of a
 * launch and writes into `label` (label_bytes bytes, NUL-terminated) the launches in order, joined by " + ", each
 *   "<kernel with its template arguments, as rocprofv3 prints it> grid <workgroups> block <threads> lds <dynamic bytes>"
 * followed by " ws <workspace bytes the arm needs>" (a call that launches nothing: "ws 0").  Dereferences no pointer (null-ness
 * and alignment are all it looks at) and touches no device; returns the non-zero code, with the error text, that the launch
 * would return before launching. */
int tt_voxel_pool_fwd_plan(int batch_size, int num_points, int num_channels,
                           int num_voxel_x, int num_voxel_y, int num_voxel_z,
                           const int32_t* geom_xyz, const float* input_features,
                           float* output_features, int32_t* pos_memo,
                           void* workspace, long long workspace_bytes, int ws_entry, char* label, int label_bytes);

/* Planned forward for STATIC geometry (fixed camera rig: the same geom_xyz every frame; closed-loop ticks, the bench).
 * tt_voxel_pool_plan_build sorts the in-range points by (sample, cell) once; tt_voxel_pool_fwd_planned then streams
 * the point rows cell by cell with no index work, no atomics, deterministic.  Same result as tt_voxel_pool_fwd
 * (output_features is accumulated into, pre-zero it like the reference does). */
long long tt_voxel_pool_plan_bytes(int batch_size, int num_points, int num_voxel_x, int num_voxel_y);
long long tt_voxel_pool_plan_workspace_bytes(int batch_size, int num_points);
int tt_voxel_pool_plan_build(int batch_size, int num_points, int num_voxel_x, int num_voxel_y, int num_voxel_z,
                             const int32_t* geom_xyz, void* workspace, long long workspace_bytes, void* plan,
                             long long plan_bytes, void* stream);
long long tt_voxel_pool_planned_workspace_bytes(int batch_size, int num_points, int num_channels, int num_voxel_x,
                                                int num_voxel_y);
int tt_voxel_pool_fwd_planned(int batch_size, int num_points, int num_channels, int num_voxel_x, int num_voxel_y,
                              const void* plan, const float* input_features, float* output_features, void* workspace,
                              long long workspace_bytes, void* stream);

/* A9: VoxelPooling.backward (ops/voxel_pooling/voxel_pooling.py:57-69):
 * grad_in[b,p,:] = grad_out[b,:,y,x] for kept points, 0 elsewhere.
 * grad_out is the [B,Y,X,C] (channel-last) view of the reference's [B,C,Y,X]. */
int tt_voxel_pool_bwd(int batch_size, int num_points, int num_channels,
                      int num_voxel_x, int num_voxel_y,
                      const int32_t* pos_memo, const float* grad_out_bhwc,
                      float* grad_in, void* stream);

/* A7 + LSS.voxel_pooling_method index math (backbones/lss.py:474-512,629-631):
 * frustum point -> ego xyz -> int voxel index (C truncation toward zero).
 * mats: per (b,cam) two 4x4 row-major f32 matrices: inv(ida) and
 * sensor2ego @ inv(intrin)   [B*ncam][2][16].
 * frustum f32 [D,fH,fW,4]; geom_xyz out int32 [B, ncam*D*fH*fW, 3].
 * voxel_lo[3] = voxel_coord - voxel_size/2, voxel_size[3]: HOST pointers (module constants). */
int tt_frustum_voxel_index(int batch_size, int num_cams, int D, int fH, int fW,
                           const float* frustum, const float* mats,
                           const float* voxel_lo, const float* voxel_size,
                           int32_t* geom_xyz, float* geom_f32_or_null,
                           void* stream);

/* A6+A8 fused: depth-softmax (x) context -> BEV without materialising the
 * [B,N,D,H,W,C] outer product (backbones/lss.py:583-615 + voxel pooling).
 * depth_logits [B*ncam, fH, fW, D] (channel-last), context [B*ncam, fH, fW, C]
 * (dtype = TT_F32 or TT_BF16), geom_xyz int32 as above,
 * out f32 [B, Y, X, out_cstride] written at channel offset out_coff, with the
 * rot90(flip) of encoder_decoder_framework.py:241 applied when rot_flip != 0.
 * out must be pre-zeroed. */
int tt_lift_splat_fwd(int batch_size, int num_cams, int D, int fH, int fW, int C,
                      int num_voxel_x, int num_voxel_y, int num_voxel_z,
                      const void* depth_logits, const void* context, int dtype,
                      const int32_t* geom_xyz, float* out, int out_cstride,
                      int out_coff, int rot_flip, void* stream);

/* Same with a caller-provided workspace (tt_lift_splat_workspace_bytes; its contents do not matter): every image strip
 * stores one partial row per BEV cell it touches plus its cell -> slot table, and a second kernel adds each cell's
 * partial rows to `out` in strip order -- no floating-point atomics, so equal inputs give bit-identical output.
 * ws == NULL, or a shape the strip kernel does not take (workspace_bytes == 0), is tt_lift_splat_fwd. */
long long tt_lift_splat_workspace_bytes(int batch_size, int num_cams, int D, int fH, int fW, int C,
                                        int num_voxel_x, int num_voxel_y);
int tt_lift_splat_fwd_ws(int batch_size, int num_cams, int D, int fH, int fW, int C,
                         int num_voxel_x, int num_voxel_y, int num_voxel_z,
                         const void* depth_logits, const void* context, int dtype,
                         const int32_t* geom_xyz, float* out, int out_cstride,
                         int out_coff, int rot_flip, void* ws, long long ws_bytes, void* stream);
/* Host only: tt_voxel_pool_fwd_plan for tt_lift_splat_fwd_ws (ws == NULL: tt_lift_splat_fwd): the per-pixel atomic kernel, the
 * strip kernel with atomics, or the strip kernel + lift_splat_cells_kernel (csrc/voxel_pool_choose.cpp: lift_splat_choose). */
int tt_lift_splat_fwd_plan(int batch_size, int num_cams, int D, int fH, int fW, int C,
                           int num_voxel_x, int num_voxel_y, int num_voxel_z,
                           const void* depth_logits, const void* context, int dtype,
                           const int32_t* geom_xyz, float* out, int out_cstride,
                           int out_coff, int rot_flip, void* ws, long long ws_bytes, char* label, int label_bytes);

/* ------------------------------------------------------------------------
 * Implicit-GEMM convolution / linear on MFMA, channel-last activations.
 *   out[n,oh,ow,co] = act( scale[co]*sum(...) + shift[co] + shift_n[n%mod,co]
 *                          + res1 + res2 )
 * Covers nn.Conv2d / nn.Linear / ConvTranspose2d(k2,s2) call sites of
 * backbones/lss.py, encoder_decoder_framework.py, dense_heads/ (all files).
 * ---------------------------------------------------------------------- */
typedef struct tt_conv_desc {
    /* input  [N, H, W, in_cstride] read at channel offset in_coff, Cin used */
    const void* in;   int N, H, W, Cin, in_cstride, in_coff;
    long long in_nstride;           /* elements between images (0 => H*W*in_cstride) */
    /* weights [Cout_total][KH][KW][Cin] (K contiguous), dtype = dtype */
    const void* weight; int Cout, KH, KW, stride, pad, dil;
    /* output [N, OH, OW, out_cstride] at channel offset out_coff */
    void* out; int OH, OW, out_cstride, out_coff;
    long long out_nstride;          /* elements between images (0 => OH*OW*out_cstride) */
    int pixel_shuffle2;             /* 1: ConvTranspose2d k2 s2: Cout = 4*Cout_real,
                                       column j=(dh*2+dw)*Cout_real+co goes to pixel (2h+dh,2w+dw) */
    /* epilogue (all f32, nullable) */
    const float* scale; const float* shift;
    const float* shift_n; int shift_n_mod;
    const void* res1; int res1_cstride, res1_coff;
    const void* res2; int res2_cstride, res2_coff;
    int act;
    int dtype;       /* TT_F32 / TT_BF16 / TT_F16: input, weight, residual storage type */
    int out_dtype;   /* storage type of out: TT_F32, the operand dtype, or (f32 operands, no residuals) TT_F16 / TT_BF16 */
    /* sparse (spconv) mode: in = feature rows [*, in_cstride]; N = upper bound of output rows,
     * H=W=OH=OW=KH=1, KW = taps; gather_idx int32 [N][KW] = input row per (output row, tap) or -1
     * (the rulebook of tt_sp_rulebook); m_dev (nullable) = device int with the live row count. */
    const int* gather_idx;
    const int* m_dev;
    /* optional split-K workspace: f32 [N*OH*OW][Cout], zero-filled by the caller.  When given and the
     * launch would occupy < 128 workgroups with a long K loop, K is split across gridDim.y and a tiny
     * finalize kernel applies the epilogue (latency-bound decoder layers with M <= a few thousand). */
    float* splitk_ws;
    /* optional (dtype == TT_F32 only): the same weights pre-split into bf16 (hi, lo) pairs, per 16 K elements
     * 64 B = [hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15] (thinktwice_amd/weights.py::split_pairs_x3).  When given
     * and the layer fits the LDS-DMA kernel it runs in "bf16x3" arithmetic -- a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on
     * the bf16 MFMA, ~1e-5 relative error, 16/3 of the f32-MFMA rate; otherwise the exact f32 path on `weight`. */
    const void* weight_x3;
    /* optional (gather mode): the tile plan of tt_sp_tile_plan for gather_idx -- output tile i covers rows
     * row_perm[256 i .. 256 i + 255] and multiplies only the taps set in the union of their masks */
    const int* row_perm;
    const unsigned* row_mask;
    /* split-K without atomics: `splitk_ws` holds this many [N*OH*OW][Cout] f32 slices (>= tt_conv2d_splitk_slices(d), no
     * zero fill needed); every K split stores its partial tile into its own slice and the finalize kernel adds the slices
     * in index order -- bit-reproducible.  0: the legacy form (one zero-filled slice, f32 atomics) */
    int splitk_slices;
    /* bf16x3 layers (weight_x3 given) whose activation tensor has no reader but bf16x3 convolutions can move the operand split
     * from the consumer's K loop (once per USE: nine times per element per column tile in a 3 x 3 layer) to the producer (once per
     * element).  "Pair format": per 16 channels 64 B = [hi c0-7 | hi c8-15 | lo c0-7 | lo c8-15] in bf16, hi = rne(v),
     * lo = rne(v - hi) -- the weights' format along the channel axis, f32-sized.  The sums are bit-identical to the f32 form.
     *   out_pair: write `out` (out_dtype TT_F32, no residuals, Cout / out_cstride / out_coff multiples of 16) in pair format;
     *   in_pair : `in` is in pair format (in_cstride / in_coff multiples of 16, Cin % 32 == 0, N*OH*OW > 4096, Cout <= 32 or
     *             >= 64): the launch is refused if the layer is outside the LDS-DMA kernel's contract. */
    int in_pair, out_pair;
    /* optional (dtype == TT_F16 only): "h2" arithmetic -- IEEE-half activations as stored x an f16 (hi, lo) weight pair, two
     * v_mfma_f32_32x32x16_f16 per product with f32 accumulation (exact to ~2^-22 with respect to the stored operands).
     * Layout: rows of 2*K halves, per 16 K elements 64 B = [hi k0-7 | hi k8-15 | lo k0-7 | lo k8-15], hi = f16(w),
     * lo = f16(w - hi) (thinktwice_amd/weights.py::split_pairs_h2).  Needs Cin % 64 == 0; `weight` is then only a shape
     * carrier.  The PAFPN of the mixed mode runs it. */
    const void* weight_h2;
    /* optional second copy of the output, always f32, rows [N*OH*OW] of out2_cstride floats at channel offset out2_coff
     * (row-linear outputs only): a layer whose result is read both by a half-storage consumer and by an f32 one
     * (PAFPN fpn_convs.0: downsample_convs.0 reads the f16 copy, the UNet concat buffer takes the f32 one) */
    float* out2; int out2_cstride, out2_coff;
    /* optional: res1 is a coarser map [N][res1_up_h][res1_up_w][res1_cstride] read through NEAREST upsampling to (OH, OW)
     * (pixel (oh, ow) adds pixel (oh * res1_up_h / OH, ow * res1_up_w / OW)): `lat[i-1] += F.interpolate(lat[i], size=...)` of the
     * PAFPN top-down path (backbones/lss.py:301-305) inside the lateral conv.  0 = res1 has the output's own geometry.  Needs the
     * vector epilogue and more than 4096 output rows. */
    int res1_up_h, res1_up_w;
    /* 1: res1 is an f32 tensor although the operands are 16-bit (dtype TT_F16 / TT_BF16): the f32 sum chains of the mixed mode's
     * PAFPN beside its half conv inputs.  Vector epilogue only. */
    int res1_f32;
    /* 1 (bf16x3 layers: dtype TT_F32, weight_x3 given): `in` is the low-resolution f32 map [N][H/2][W/2][Cin] and the layer reads it
     * THROUGH nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True): H, W (both even) describe the upsampled, logical input,
     * which never exists in memory.  The result is bit for bit that of tt_bilinear_up2_pair followed by the same layer with in_pair.
     * Contract: 3 x 3, stride 1, pad 1, dil 1 (OH = H, OW = W), Cin % 32 == 0, Cout == 64, N*OH*OW > 4096, a contiguous source
     * (in_cstride = Cin, in_coff = 0, in_nstride 0 or (H/2)*(W/2)*Cin), the vector epilogue; no residual, per-image shift, out2,
     * split-K workspace or in_pair (out_pair is fine).  Anything else is refused with an error, never run on another kernel. */
    int in_up2;
} tt_conv_desc;

/* The two row counts callers route by (csrc/conv_choose.h derives its bounds from them; thinktwice_amd/ops.py reads them here).
 * TT_CONV_SMALL_ROWS: up to this many output rows a plain dense layer runs the exact-f32 latency kernel (conv_small.hip), whose
 * sums no bf16x3 form reproduces, so "N*OH*OW > 4096" in the contracts above and below is "more than TT_CONV_SMALL_ROWS".
 * TT_CONV_JOIN_MIN_ROWS: fewest rows from which every routed form of a joined stage (tt_conv_next) beats its two launches. */
#define TT_CONV_SMALL_ROWS 4096
#define TT_CONV_JOIN_MIN_ROWS 32768

/* A JOINED STAGE for tt_conv2d_fwd_next (bf16x3 layers: dtype TT_F32, weight_x3 given): the 1 x 1 / stride 1 convolution that reads the
 * layer's output runs in the SAME launch, on each row tile of `out` while it is still on chip,
 *   next_out = next_act(next_scale * (next_weight . out) + next_shift),
 * so `out` (still written: it has other readers) is not read back.  Both tensors are, bit for bit, those of tt_conv2d_fwd(d) followed
 * by tt_conv2d_fwd of the second layer on `out` (a ResNet bottleneck's conv3 and the next block's conv1).  (Its own struct and entry,
 * beside tt_conv_desc: the descriptor's layout stays what its callers were built against.)
 *   next_weight     f32 [next_cout][1][1][Cout]: only the shape carrier, as `weight` is for a bf16x3 layer;
 *   next_weight_x3  the same in pair format (see tt_conv_desc.weight_x3), 16-byte aligned: what the kernel reads;
 *   next_scale / next_shift  folded BN of the second layer (nullable: 1 / 0);  next_act  TT_ACT_NONE or TT_ACT_RELU;
 *   next_out        [N, OH, OW, next_out_cstride] at channel offset next_out_coff, 64-byte aligned, contiguous images;
 *   next_out_pair   must be 1: next_out is written in pair format (out_pair's rules: next_cout / next_out_cstride / next_out_coff
 *                   multiples of 16).
 * Contract of the layer `d`: 1 x 1, stride 1, pad 0 (OH = H, OW = W), Cin = 64, 128 or 256, Cout = 4 Cin, with next_cout = 64 or 128
 * (Cin = 64), 128 or 256 (Cin = 128), 256 (Cin = 256); `in` f32 or in_pair, row-linear (in_nstride 0 or H*W*in_cstride; in_pair:
 * in_cstride / in_coff multiples of 16); `out` f32 (no out_pair), row-linear, the vector epilogue; at most res1 (f32, 16-byte
 * aligned rows, its own res1_cstride / res1_coff); act TT_ACT_NONE or TT_ACT_RELU; N*OH*OW > 4096 (it pays from kJoinMinRows =
 * 32,768 rows on, csrc/conv_choose.h: below, tt_conv_last_kernel's label ends in " below kJoinMinRows"); no res2, shift_n, out2,
 * res1_up_*, split-K workspace, gather or pixel shuffle.  Each stage alone, at this row count, must run on a bf16x3 LDS-DMA tile (no
 * split-K, not the exact-f32 path): those are the kernels whose sums the joined kernel reproduces.  Anything outside this is refused
 * with an error naming the field; tt_conv2d_fwd_next never runs as two launches. */
typedef struct tt_conv_next {
    const void* next_weight; const void* next_weight_x3;
    int next_cout;
    const float* next_scale; const float* next_shift;
    int next_act;
    void* next_out; int next_out_cstride, next_out_coff;
    int next_out_pair;
} tt_conv_next;

int tt_conv2d_fwd(const tt_conv_desc* d, void* stream);
/* tt_conv2d_fwd of `d` with the joined stage `next` (non-null) in the same launch: the contract above. */
int tt_conv2d_fwd_next(const tt_conv_desc* d, const tt_conv_next* next, void* stream);
/* K splits tt_conv2d_fwd would use for this descriptor if it is given a split-K workspace (0: the layer does not split).  Asks the
 * dispatch function of a launch, so a descriptor whose launch would be refused (tt_conv2d_plan != 0: out2 / res1 without the vector
 * epilogue, a misaligned weight_x3, ...) answers 0 and leaves that refusal in tt_last_error. */
int tt_conv2d_splitk_slices(const tt_conv_desc* d);
/* Host only: which kernel tt_conv2d_fwd would run `d` on.  Runs the validation and the dispatch of a launch (csrc/conv_choose.cpp) and
 * writes into `label` (label_bytes bytes, NUL-terminated) what tt_conv_last_kernel would report after that launch.  Dereferences no
 * data pointer of the descriptor (null-ness and alignment are all it looks at) and touches no device; returns the non-zero code, with
 * the error text, that the launch of `d` would return before launching. */
int tt_conv2d_plan(const tt_conv_desc* d, char* label, int label_bytes);
/* the same for tt_conv2d_fwd_next(d, next, ..) */
int tt_conv2d_plan_next(const tt_conv_desc* d, const tt_conv_next* next, char* label, int label_bytes);

/* Two 1 x 1 convolutions with folded BN over the R rows of a row matrix in ONE launch (seg_res_to_image_feature.0 / .3,
 * backbones/lss.py:409-416, over the full-resolution segmentation map):
 *   y = act1(scale1 * (W1 . x) + shift1)   K1 -> 64        z = act2(scale2 * (W2 . y) + shift2)   64 -> N2
 * The 64-wide intermediate never reaches global memory.  The result is bit for bit that of the two tt_conv2d_fwd launches
 * (stage 1: weight = w1, no weight_x3; stage 2: weight = w2, weight_x3 = w2_x3) over the same R rows: each stage runs the
 * arithmetic the convolution dispatch picks for it at this row count (exact f32 up to 65,535 rows, bf16x3 on stage 2 beyond).
 * x: f32 rows of x_stride floats, the first K1 read (K1 = 16, or 12: columns 12-15 are then zeros, as tt_conv2d_fwd pads its K);
 * w1 f32 [64][K1]; w2 f32 [N2][64] and w2_x3 the same in pair format (tt_conv_desc.weight_x3); N2 = 8, 16 or 32; scale / shift
 * f32 per output channel, nullable; act1 / act2 TT_ACT_NONE or TT_ACT_RELU; out f32 rows of out_stride floats, written at
 * channel offset out_coff.  Strides and offsets are multiples of 4 and every pointer is 16-byte aligned; anything else returns
 * an error before the launch. */
int tt_seg_feedback_chain(const float* x, long long R, int x_stride, int K1, const float* w1, const float* scale1,
                          const float* shift1, int act1, const float* w2, const void* w2_x3, int N2, const float* scale2,
                          const float* shift2, int act2, float* out, int out_stride, int out_coff, void* stream);

/* ------------------------------------------------------------------------
 * A chain of nn.Linear layers over R rows in ONE launch (the decoder's row-batched MLPs:
 * thinktwice_decoder.py:26-260 query_linear / ffn / output_proj / mlp / traj_offset_module / ctrl_offset_module /
 * flattened_BEV_feat_update_module and the coarse heads :419-445; MSDA sampling_offsets / attention_weights,
 * multi_scale_deformable_attn_function.py:431-447).  A workgroup owns 32 rows and walks the whole chain with the
 * intermediates in LDS; bf16x3 arithmetic (see tt_conv_desc.weight_x3).
 *   stage s:  y = act( W_s . in + bias + side_w . side[m, :side_k] + res[m, res_coff + n] )
 *   in = the chain input x (in_sel = -1) or the output of an earlier stage (in_sel = its index)
 * w: pair-format weights [N rounded up to 32][Kp] (weights.py::split_pairs_x3 of the zero-padded f32 matrix),
 * Kp % 16 == 0.  `out` (nullable): f32 rows in global memory.  Outputs that a later stage reads stay in LDS
 * (<= 160 KiB in total per 32 rows, checked).
 * Two forms, tt_mlp_chain and tt_mlp_chain_wide below; both entries are FORCED forms (what a launch plan records).  Which one a
 * chain should take, with which grid, and every argument check of both: csrc/chain_choose.cpp, asked through tt_mlp_chain_plan.
 * ---------------------------------------------------------------------- */
typedef struct tt_chain_stage {
    const void* w; const float* bias;
    int K, Kp, N, act, in_sel;
    const float* res; int res_stride, res_coff;
    const float* side; const float* side_w; int side_stride, side_k;
    float* out; int out_stride, out_coff;
} tt_chain_stage;
/* n_split > 1 (single stage only): the N columns are dealt over n_split workgroups per 32 rows (few rows, wide N:
 * the BEV update's broadcast-channel term, 2048 -> 9 x 128) */
int tt_mlp_chain(const float* x, long long R, int x_stride, int nstages, const tt_chain_stage* stages, int n_split,
                 void* stream);
/* The same chain for FEW rows (the batch-1 tick: 1 - 32 rows, where a chain's time is the latency of streaming its weights
 * through one workgroup): the 32-column blocks of every stage are dealt over `n_groups` co-resident workgroups per 32 rows, the
 * waves of a workgroup split K; stage outputs a later stage reads go through `workspace` (f32, global) and the workgroups of
 * a row block meet at a ticket barrier between dependent stages.  Same arithmetic per product as tt_mlp_chain (bf16x3), the K
 * sum is taken in eight interleaved slices added in a fixed order.
 * Co-residency: the barrier needs every workgroup of the launch running.  The library bounds a launch to
 * tt_mlp_chain_wide_max_workgroups() = (hipOccupancyMaxActiveBlocksPerMultiprocessor x CUs) / 2 workgroups (two launches at a
 * time: the decoder's main and branch streams) and returns -1 beyond it (tt_mlp_chain_plan never chooses such a grid).  A wait
 * is bounded; a wait that gives up is LOUD: the workgroup writes NaN from there on, the device's fault word (pinned host memory,
 * written by the kernel; tt_dec_gru's hand-over shares it) is set, and from then on tt_mlp_chain_wide, tt_dec_gru, tt_plan_run,
 * tt_encoder_fwd and tt_decoder_fwd return -3 until tt_clear_device_faults().
 * tt_device_faults(): non-blocking read of that word for the current device (check it after any
 * synchronisation with the forward's streams -- thinktwice_amd does after the D2H copy of tt_action_post's result and at the
 * start of every forward); tt_mlp_chain_wide_faults(): the same after a hipDeviceSynchronize().  Ticket counters are per
 * device; launches recorded into a HIP graph claim theirs permanently (a replay reuses the recorded counter); when those
 * are used up the call returns -4 (nothing launched): record tt_mlp_chain instead. */
long long tt_mlp_chain_wide_workspace_bytes(long long R, int nstages, const tt_chain_stage* stages);
int tt_mlp_chain_wide(const float* x, long long R, int x_stride, int nstages, const tt_chain_stage* stages, int n_groups,
                      void* workspace, long long workspace_bytes, void* stream);
int tt_mlp_chain_wide_max_workgroups(void);
/* What a chain of these rows and stages runs as.  Host arithmetic only: touches no device and dereferences no data pointer (the
 * stages' pointers are tested for null-ness and alignment), takes no stream (a launch plan does not record it), and returns the
 * code and error text the launch would return before launching.  force: 0 by the rows (the wide form up to 512 rows, unless
 * TT_CHAIN_WIDE=0 or the device cannot hold a workgroup per row group), 1 tt_mlp_chain, 2 tt_mlp_chain_wide with `groups` clamped to
 * what can be co-resident, 3 tt_mlp_chain_wide with exactly `groups` (refused beyond the bounds, as the entry does).  groups: column
 * groups wanted, 0 = the widest stage's 32-column blocks, at most 16.  n_split: tt_mlp_chain's.  max_workgroups: what
 * tt_mlp_chain_wide_max_workgroups() answered on the device the chain will run on.
 * Answer: wide (0: call tt_mlp_chain with n_split; 1: tt_mlp_chain_wide with n_groups and a workspace of workspace_bytes), the
 * launch's grid row_groups x (n_groups | n_split) and its dynamic LDS. */
typedef struct tt_chain_choice {
    long long row_groups, workspace_bytes, dynamic_lds;
    int wide, n_groups, n_split;
} tt_chain_choice;
int tt_mlp_chain_plan(long long R, int x_stride, int nstages, const tt_chain_stage* stages, int n_split, int groups, int force,
                      int max_workgroups, tt_chain_choice* out);
int tt_mlp_chain_wide_faults(void);
int tt_device_faults(void);
int tt_clear_device_faults(void);
/* test hook: polls before a barrier wait gives up (default 1 << 21, about a second; 0 forces a time-out; < 0 restores) */
int tt_mlp_chain_wide_set_max_spin(int polls);
/* debug: while set, every tt_mlp_chain_wide workgroup writes up to 64 wall-clock stamps (10 ns ticks; kernel entry, then per stage:
 * entry, barrier passed, first block's K loop + reduction done, stage done) at stamps[(row_group * n_groups + group) * 64] */
int tt_mlp_chain_wide_set_trace(void* stamps_or_null);

/* ------------------------------------------------------------------------
 * Spatial half of a refinement layer as persistent per-sample kernels (csrc/dec_spatial.hip), bf16x3 arithmetic.
 * All weight tensors are pair format (weights.py::split_pairs_x3), K order tap-major / channel-minor.
 * ---------------------------------------------------------------------- */
/* SpatialGRU (dense_heads/utils.py:53-106): inp6 [B][4][6] (waypoint xy, softplus ctrl), state [B][441][32] f32
 * channel-last -> fut [B][4][441][32].  w0/wx/b0/w2/b2: arrays of 3 (conv_update, conv_reset, conv_state_tilde):
 * w0 = state part of the .0 conv [32][9*32], wx = its constant-input part f32 [9][6][32], w2 = the .2 conv.
 * scratch: tt_dec_gru_scratch_floats(B) floats ([B][3][448][32] f32 -- the 441 pixels padded to 14 row blocks of 32 -- + two flag
 * words per sample: two workgroups per sample hand the state and the update gate over through it; a hand-over that times out
 * sets the device fault word, tt_device_faults). */
long long tt_dec_gru_scratch_floats(int B);
int tt_dec_gru(int B, const float* inp6, const float* state, float* fut, float* scratch, const void* const* w0,
               const float* const* wx, const float* const* b0, const void* const* w2, const float* const* b2,
               const void* wd0, const float* bd0, const void* wd2, const float* bd2, void* stream);
/* grid2feat (encoder_decoder_framework.py:228-234, thinktwice_decoder.py:405-415): maps x [441][32] -> [256];
 * 17 weight sets in the order documented in dec_spatial.hip; mids (nullable): the three SE-block outputs;
 * scratch: tt_dec_flatten_scratch_floats(maps) floats (the tensors between the per-layer launches of the 4x4 level on). */
long long tt_dec_flatten_scratch_floats(int maps);
int tt_dec_flatten(int maps, const float* in, float* out, float* mids_or_null, float* scratch, const void* const* w,
                   const float* const* b, const float* bn_scale, const float* bn_shift, void* stream);
/* debug: while set, workgroup 0 of tt_dec_gru / tt_dec_flatten writes a wall-clock stamp (10 ns ticks) after every phase (<= 64) */
int tt_dec_set_trace(void* stamps_or_null);
/* BEV_feat_update_module + residual (thinktwice_decoder.py:221-225,257): bev [B][441][32], G [B][9][128] = the
 * broadcast-channel term per tap (tt_mlp_chain over h), w0 [128][9*32] (bev part), w2[4] [32][9*32] per hidden chunk;
 * scratch: tt_dec_bev_update_scratch_floats(B) floats (the four hidden-channel chunks' partial maps + a ticket per sample). */
long long tt_dec_bev_update_scratch_floats(int B);
int tt_dec_bev_update(int B, const float* bev, const float* G, float* out, long long out_bstride, float* out2,
                      long long out2_bstride, float* scratch, const void* w0, const float* b0, const void* const* w2,
                      const float* b2, void* stream);

/* ------------------------------------------------------------------------
 * HBM-bound glue of the forward (channel-last; `dtype` = storage type of the activation).
 * Each replaces a torch call of the reference forward (call sites cited).
 * ---------------------------------------------------------------------- */
/* img (B*T*N,3,H,W) f32 NCHW -> channel-last with zero-padded channels (lss.py:517-519) */
int tt_nchw_to_nhwc_pad(const float* in, void* out, int N, int C, int H, int W, int Cp,
                        int out_dtype, void* stream);
/* Same conversion into the interior of a spatially padded buffer out[N][Hp][Wp][Cp] at pixel offset (top, left);
 * the border is NOT written (allocate it zeroed once).  Feeds the row-run form of the 7x7/2 ResNet stem, whose 8-pixel
 * input runs overhang the image (reference: mmdet ResNet.conv1 via backbones/lss.py:517-519 get_cam_feats). */
int tt_nchw_to_nhwc_border(const float* in, void* out, int N, int C, int H, int W, int Cp, int Hp, int Wp,
                           int top, int left, int out_dtype, void* stream);
/* channel-last -> NCHW f32 (outputs returned in the reference layout) */
int tt_nhwc_to_nchw(const void* in, float* out, int N, int C, int H, int W, int cstride, int coff,
                    int in_dtype, void* stream);
/* F.max_pool2d(x,3,2,1): mmdet ResNet stem (lss.py:401 -> [3P]) */
int tt_maxpool3x3s2(const void* in, void* out, int N, int H, int W, int C, int dtype, void* stream);
/* The ResNet stem of the bf16x3 modes in ONE launch, from the NCHW image to the pooled map (csrc/conv_x3_stem.hip):
 *   out = F.max_pool2d(relu(scale * conv7x7s2p3(img) + shift), 3, 2, 1)   f32 (B*T*N, ceil(H/4), ceil(W/4), 64), channel-last, contiguous
 * bit for bit what tt_nchw_to_nhwc_border (4 channels, border 3 / 3 / 3 / 5), tt_conv2d_fwd of the row-run stem (7 x 1, stride 2,
 * in_cstride 4, ReLU) and tt_maxpool3x3s2 produce over the same image.  Inference only.
 *   img          f32 (B, T, N, 3, H, W): element (b, t, n, c, y, x) at img[b*stride_b + t*stride_t + n*stride_n + c*stride_c +
 *                y*stride_h + x*stride_w]; the inner (3, H, W) block must be contiguous (stride_c = H*W, stride_h = W, stride_w = 1),
 *                H and W even.  Output image (s*B + b)*N + n is img[b, T-1-s, n] (sweep-major, key sweep first).  img_dtype: TT_F32.
 *   weight_x3    the row-run stem weights f32 [w_cout = 64][w_kh = 7][1][w_k = 32] (8 pixels x 4 channels per filter row, the 4th
 *                channel and the 8th pixel zero) in pair format (tt_conv_desc.weight_x3), 16-byte aligned;
 *   scale/shift  folded BN, 64 floats each;  out: 16-byte aligned, out_floats = the floats it may hold;
 *   max_workgroups  0, or a bound on the persistent grid (tests).
 * Anything else is refused with an error naming the field; nothing here runs as three launches. */
int tt_stem_pool_x3(const float* img, long long stride_b, long long stride_t, long long stride_n, long long stride_c,
                    long long stride_h, long long stride_w, int B, int T, int N, int H, int W, int img_dtype,
                    const void* weight_x3, int w_cout, int w_kh, int w_k, const float* scale, const float* shift,
                    float* out, long long out_floats, int max_workgroups, void* stream);
/* dst += F.interpolate(src, size=dst.shape, mode='nearest'): PAFPN top-down (lss.py:301-305) */
int tt_upsample_nearest_add(void* dst, const void* src, int N, int H, int W, int C, int h, int w,
                            int dtype, void* stream);
/* nn.Upsample(scale_factor=2, bilinear, align_corners=True): UNet (lss.py:267) */
int tt_bilinear_up2(const void* in, void* out, int N, int H, int W, int C, int dtype, void* stream);
/* the same, f32 in -> bf16x3 pair format out (tt_conv_desc.in_pair of the consuming convolution; C % 16 == 0) */
int tt_bilinear_up2_pair(const float* in, float* out, int N, int H, int W, int C, void* stream);
/* mode 0: AdaptiveAvgPool2d(1) (lss.py:80); mode 1: 0.5*mean+0.5*max (code/utils.py:91-92); out f32 [N,C] */
int tt_spatial_pool(const void* in, float* out, int N, int HW, int C, int cstride, int coff, int mode,
                    int dtype, void* stream);
/* out = out_act(x * gate_act(gate[n,c]) + res): SELayer (lss.py:158), SEModule+residual (utils.py:96,117-119) */
int tt_channel_gate(const void* x, const float* gate, const void* res, void* out, int N, int HW, int C,
                    int gate_act, int out_act, int dtype, void* stream);
/* rows: out = act(x*scale[c] + shift[c]): eval BatchNorm1d (lss.py:232, encoder_decoder_framework.py:134) */
int tt_affine_rows(const void* x, const float* scale, const float* shift, void* out, long long R, int C,
                   int x_stride, int out_stride, int act, int dtype, void* stream);
/* nn.LayerNorm over the last dim (MSDA:252,201,262; thinktwice_decoder.py:197) */
int tt_layernorm_rows(const void* x, const float* gamma, const float* beta, void* out, long long R,
                      int D, int x_stride, int out_stride, float eps, int dtype, void* stream);
/* strided channel-offset copy (torch.cat assembly); rot_flip!=0: torch.rot90(torch.flip(x,[2]),1,[2,3])
 * (encoder_decoder_framework.py:241,246) */
int tt_copy_nhwc(const void* in, void* out, int N, int H, int W, int C, int in_cstride, int in_coff,
                 int out_cstride, int out_coff, int rot_flip, int in_dtype, int out_dtype, void* stream);
/* out[n,p,coff+c] = v[n,c]: `.unsqueeze(-1).unsqueeze(-1).repeat` (thinktwice_decoder.py:42,257) */
int tt_broadcast_rows(const void* v, void* out, int N, int HW, int C, int v_stride, int out_cstride,
                      int out_coff, int dtype, void* stream);
/* op 0: a+b; 1: (1-b)*a; 2: (1-g)*a+g*b; 3: act(a)   (SpatialGRU.gru_cell, dense_heads/utils.py:93-106) */
int tt_ew(const void* a, const void* b, const void* g, void* out, long long R, int C, int a_stride,
          int a_coff, int b_stride, int b_coff, int g_stride, int g_coff, int o_stride, int o_coff,
          int op, int act, int dtype, void* stream);
/* torch.cat([...], -1) of up to 8 row-batched f32 pieces in one launch (decoder MLP inputs, thinktwice_decoder.py:
 * 236-260): piece s writes out[r, coffs[s] : coffs[s]+widths[s]] = srcs[s][((r / divs[s]) % mods[s]) * strides[s] + c]
 * (mods[s] = 0: no modulo; srcs[s] = NULL: zeros).  Pieces are contiguous in output-column order.  All arrays HOST. */
int tt_concat_rows(float* out, long long R, int out_stride, int nseg, const float* const* srcs, const int* strides,
                   const int* widths, const int* coffs, const int* divs, const int* mods, void* stream);

/* mmcv DeformConv2dPack (DCN v1, 3x3, stride 1, deform_groups 1) column builder (lss.py:189-197):
 * cols [N*H*W, 9, C] = bilinear samples of x [N,H,W,C] at the offset taps; offsets f32
 * [N,H,W,off_cstride] with channels [dy_0,dx_0,...,dy_8,dx_8].  The grouped GEMM runs on tt_conv2d_fwd. */
int tt_deform_im2col3x3(const void* x, const float* offsets, void* cols, int N, int H, int W, int C,
                        int off_cstride, int pad, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * Look module (dense_heads/thinktwice_decoder.py:88-187 + multi_scale_deformable_attn_function.py).
 * All per-(sample,camera) query packing stays on the device (the reference does B*4 nonzero()
 * host syncs per decoder layer, thinktwice_decoder.py:131-137).  120 slots are always computed;
 * `max_len` (device int) bounds the final reduction exactly like the reference's padded length.
 * ---------------------------------------------------------------------- */
/* obtain_cam_ref_points_query (DEC:89-113,129-149): wp (B,4,2); lidar2img/ida_mat (B,4,4,4) f32.
 * -> ref_packed (B,4,120,2), query_of_slot (B,4,120) (-1 = padded), count (B,4), max_len (1). */
int tt_look_project_pack(int B, const float* wp, const float* lidar2img, const float* ida_mat,
                         float img_h, float img_w, float* ref_packed, int* query_of_slot,
                         int* count, int* max_len, void* stream);
/* query rows (B*4*120, row_stride>=1543) f32 = [ctrl 4 | xyz 3 | emb 128 | meas 128 | flat 256 |
 * F.grid_sample of the 4 fpn_linear maps (c*4+lvl) 1024] (DEC:119-127,148,164-171); padded slots = 0.
 * level_maps: 4 HOST-array device pointers to [B*4,H_l,W_l,256] maps; level_hw: 8 host ints. */
int tt_look_gather_query(int B, const int* query_of_slot, const float* ref_packed, const float* wp,
                         const float* ctrl_softplus, const float* temporal_embedding,
                         const float* static_embedding, const float* measurement_feat,
                         const float* flattened_feat, const void* const* level_maps,
                         const int* level_hw, int maps_dtype, float* out, int row_stride, void* stream);
/* MSDeformableAttention3D core (MSDA:478-526 + mmcv multi_scale_deformable_attn_pytorch [3P]):
 * value [B*4, sum(HW), 256] (8 heads x 32), offsets f32 [R,512], logits f32 [R,256], R = B*4*120. */
int tt_msda_sample(int B, const void* value, int value_dtype, const float* offsets, const float* logits,
                   const float* ref_packed, const int* level_hw, float* out, void* stream);
/* Same core over a value tensor whose rows hold `value_cstride` >= 256 channels, sampling the 256-channel window at
 * `value_coff`: lets ONE value-projection GEMM (Cout = layers x 256) serve all five refinement layers, each layer's
 * attention reading its own window (the reference projects per layer, thinktwice_decoder.py:392-398 inside the loop
 * of 428-447; the projections only depend on the FPN maps). */
int tt_msda_sample_strided(int B, const void* value, int value_dtype, int value_cstride, int value_coff,
                           const float* offsets, const float* logits, const float* ref_packed, const int* level_hw,
                           float* out, void* stream);
/* SpatialCrossAttention "mask & average" incl. its batch-coupling bug (MSDA:338-342):
 * out (B, 4*256) = sum_{s=B}^{max_len-1} x[b,cam,s,:] / B. */
int tt_sca_reduce(int B, const float* x, const int* max_len, float* out, void* stream);

/* Composite-decoder variants of the four row producers above with the nn.LayerNorm that follows them folded in
 * (query_linear.0 thinktwice_decoder.py:131, ffn.norm MSDA:262, output_proj.0 DEC:141, mlp.0 DEC:197): each output
 * feeds tt_mlp_chain directly.  tt_look_query_ln: `ctrl` raw (raw_ctrl=1: softplus applied here) or softplus'ed. */
int tt_look_query_ln(int B, const int* query_of_slot, const float* ref_packed, const float* wp, const float* ctrl,
                     int raw_ctrl, const float* temporal_embedding, const float* static_embedding,
                     const float* measurement_feat, const float* flattened_feat, const void* const* level_maps,
                     const int* level_hw, int maps_dtype, const float* gamma, const float* beta, float eps, float* out,
                     int row_stride, void* stream);
int tt_msda_sample_ln(int B, const void* value, int value_dtype, int value_cstride, int value_coff,
                      const float* offsets, const float* logits, const float* ref_packed, const int* level_hw,
                      const float* gamma, const float* beta, float eps, float* out, float* out_ln,
                      const int* max_len_or_null, void* stream);
/* The same rows WITHOUT a projected value tensor ("sample first, project after"): level_maps = the four fpn_linear maps
 * [B*4][H_l][W_l][256] f32, wvT = value_proj.weight transposed [in 256][out 256], bias [256], vshift [level 4][camera 4][256] =
 * W (cams_embeds + level_embeds) (thinktwice_decoder.py:392-393).  value_proj is applied to the attention-weighted sum of the raw
 * rows; the bias / embedding terms enter through the in-bounds weight of each level (zero padding).  Replaces
 * multi_scale_deformable_attn_function.py:474 (value_proj over every position) + :497-525 in the composite decoder. */
int tt_msda_sample_proj_ln(int B, const void* const* level_maps, const int* level_hw, const float* offsets,
                           const float* logits, const float* ref_packed, const float* wvT, const float* bias,
                           const float* vshift, const float* gamma, const float* beta, float eps, float* out,
                           float* out_ln, const int* max_len_or_null, void* stream);   /* max_len (device, from tt_look_project_pack): rows of
                      slots >= *max_len are skipped and left unwritten -- tt_sca_reduce_ln never reads them */
int tt_sca_reduce_ln(int B, const float* x, const int* max_len, const float* gamma, const float* beta, float eps,
                     float* out, void* stream);
/* row (b, t) of the refinement layer's mlp input: LayerNorm(cat([fflat(b,t) | look(b) | 0 | temporal(t) | meas(b)])) */
int tt_dec_merge_in(int B, const float* fflat, const float* look, const float* temporal_embedding,
                    const float* measurement_feat, const float* gamma, const float* beta, float eps, float* out,
                    void* stream);

/* ------------------------------------------------------------------------
 * LiDAR branch (backbones/lidarnet.py:87-96; bodies are third-party: mmcv Voxelization, mmdet3d
 * HardSimpleVFE / SparseEncoder, spconv).  Active-row counts live in DEVICE ints; every kernel is
 * launched over an upper bound (`max_*`) and exits early, so there is no host synchronisation
 * (the reference syncs at lidarnet.py:90 `coors[-1,0]+1`).  coords are int32 (b,z,y,x).
 * ---------------------------------------------------------------------- */
long long tt_lidar_voxelize_workspace_bytes(long long num_points_total);
/* hard voxelisation + mean VFE: points f32 [B,Np,nfeat]; pc_range_lo / voxel_size: 3 HOST floats;
 * grid_xyz: 3 HOST ints; voxels with z index >= z_limit are dropped (sparse_shape z, CFG:170).
 * -> voxel_feats f32 [<=B*Np, nfeat] (mean of the first <=max_points points in point order),
 *    coords int32 [<=B*Np,4], num_voxels (device int). */
int tt_lidar_voxelize(const float* points, int B, int Np, int nfeat, const float* pc_range_lo,
                      const float* voxel_size, const int* grid_xyz, int z_limit, int max_points,
                      void* workspace, long long workspace_bytes, float* voxel_feats, int* coords,
                      int* num_voxels, void* stream);
/* the same with mmcv's max_voxels cap: voxels are created in order of first appearance (point order) and at most
 * `max_voxels` per sample exist; points of later voxels are dropped (configs/thinktwice.py:161-165: 120000 train / 160000
 * eval; call site backbones/lidarnet.py:88).  Needed only when a sample holds more points than the cap (else
 * tt_lidar_voxelize gives the same rows); rows come out in cell order like there */
long long tt_lidar_voxelize_capped_workspace_bytes(long long num_points_total);
int tt_lidar_voxelize_capped(const float* points, int B, int Np, int nfeat, const float* pc_range_lo, const float* voxel_size,
                             const int* grid_xyz, int z_limit, int max_points, int max_voxels, void* workspace,
                             long long workspace_bytes, float* voxel_feats, int* coords, int* num_voxels, void* stream);
/* dense index volume of one resolution level: vol int32 [batch, D, H, W] = feature row or -1 */
int tt_sp_volume_build(const int* coords, const int* num_rows, long long max_rows, int batch,
                       const int* dims_zyx, int* vol, void* stream);
/* spconv SparseConv3d output-site generation (bitmap of the output cells: mark + popcount + compact; rows come
 * out in cell order); kernel_stride_pad = {kz,ky,kx,sz,sy,sx,pz,py,px} (host).  Also fills the OUTPUT level's volume. */
long long tt_sp_strided_outputs_workspace_bytes(long long out_cells);
int tt_sp_strided_outputs(const int* in_coords, const int* in_rows, long long max_in, int batch,
                          const int* kernel_stride_pad, const int* out_dims_zyx, void* workspace,
                          long long workspace_bytes, int* out_vol, int* out_coords, int* out_rows,
                          long long max_out, void* stream);
/* nbr[o][k] = input row feeding output o through tap k, or -1 (SubM: out coords == in coords) */
int tt_sp_rulebook(const int* out_coords, const int* out_rows, long long max_out,
                   const int* kernel_stride_pad, const int* in_dims_zyx, const int* in_vol, int* nbr,
                   void* stream);
/* the sparse convolution itself = tt_conv2d_fwd with gather_idx = this rulebook (MFMA gathered GEMM) */
/* Tile plan of a rulebook for the mask-sorted gathered GEMM: row_perm = the output rows sorted by their tap-occupancy
 * mask (bit t = tap t has an input), row_mask_sorted = the masks in that order (rows beyond *num_rows: 0xFFFFFFFF, last).
 * A 256-row tile of the sorted order then visits only the UNION of its rows' taps instead of all KV (spconv's
 * "implicit GEMM with mask sort"); pairs (nullable, pre-zeroed) += the number of existing (row, tap) pairs. */
long long tt_sp_tile_plan_workspace_bytes(long long max_rows);
int tt_sp_tile_plan(const int* nbr, const int* num_rows, long long max_rows, int KV, void* workspace,
                    long long workspace_bytes, int* row_perm, unsigned* row_mask_sorted,
                    unsigned long long* pairs_or_null, void* stream);
/* SparseConvTensor.dense() + view(N, C*D, H, W) (lidarnet.py:53-56), channel-last: dense
 * [B, H, W, C*D] with channel c*D+z; `dense` must be pre-zeroed. */
int tt_sp_to_dense(const void* feats, const int* coords, const int* num_rows, long long max_rows, int C,
                   const int* dims_zyx, void* dense, int dtype, void* stream);

/* ------------------------------------------------------------------------
 * fused camera preprocessing (undistort grid_sample + bilinear resize + crop + /255 +
 * ImageNet normalise; datasets/pipelines/transform.py:283-286,346-356,144,163) in one gather kernel.
 * raw uint8 [NI,H,W,3]; mapx/mapy f32 [H,W] = cv2.initUndistortRectifyMap output (pixel units);
 * mean3/std3: HOST floats.  Writes channel-last out_nhwc [NI,out_h,out_w,Cp] (dtype) and/or NCHW f32.
 * ---------------------------------------------------------------------- */
int tt_preprocess_images(const uint8_t* raw_hwc, int num_images, int H, int W, const float* mapx,
                         const float* mapy, int resized_h, int resized_w, int crop_y, int crop_x,
                         int out_h, int out_w, const float* mean3, const float* std3, void* out_nhwc,
                         int out_channels_padded, int out_dtype, float* out_nchw_or_null, void* stream);

/* ------------------------------------------------------------------------
 * The TRAINING image pipeline: IDAImageTransform(is_train=True) (configs/thinktwice.py:238-240;
 * datasets/pipelines/transform.py:248-263 the draw, :275-341 its application) + ImageTransformMulti(aug=False)
 * (:144,163).  Every camera of a sample has its own resize / crop / flip; both sweeps of the camera and its depth and
 * segmentation label maps share it.
 *
 * Parameter table: `sets` is a HOST pointer to B * N tt_ida_set, entry b * N + n for camera n of sample b (image (b, t, n) of
 * the frames and label map (b, n) both use it).  The entry checks every set and copies the table into the kernel's
 * arguments (passed by value: no device buffer, no copy, the caller may reuse the memory on return), which bounds it to
 * TT_IDA_MAX_SETS sets per call.  Returns an error, before any launch, for a non-positive resized size, crop_x < 0,
 * crop_y < 0, crop_x + out_w > resized_w, crop_y + out_h > resized_h or a flip that is not 0 / 1.
 *
 * Per output pixel (oy, ox), tt_preprocess_images' arithmetic: cx = flip ? out_w - 1 - ox : ox; source coordinate
 * (oy + crop_y + 0.5) * H / resized_h - 0.5 (and likewise along x with cx), clamped at 0, neighbours clamped at the last row /
 * column, each tap a zero-padded bilinear read of the raw image through the undistortion map.  One launch, no
 * synchronisation, no allocation.
 * ---------------------------------------------------------------------- */
#define TT_IDA_MAX_SETS 64
typedef struct tt_ida_set {
    int resized_h, resized_w;   /* resize_dims of sample_ida_augmentation, (int(H * resize), int(W * resize)) */
    int crop_y, crop_x;         /* crop origin in the resized image (crop[1], crop[0]) */
    int flip;                   /* 1: horizontal flip after the crop (torch.flip(img, [-1])) */
} tt_ida_set;
/* frames: transform.py:280-283 (undistortion), img_transform :346-358 (T.Resize, crop, flip), :163 (/255, Normalize).
 * raw uint8 [B,T,N,H,W,3]; mapx/mapy f32 [H,W] as for tt_preprocess_images; mean3/std3: HOST floats.  Writes channel-last
 * out_nhwc [B*T*N,out_h,out_w,Cp] (dtype) and/or NCHW f32 [B*T*N,3,out_h,out_w]. */
int tt_preprocess_images_ida(const uint8_t* raw_hwc, int B, int T, int N, int H, int W, const float* mapx,
                             const float* mapy, const tt_ida_set* sets, int out_h, int out_w, const float* mean3,
                             const float* std3, void* out_nhwc, int out_channels_padded, int out_dtype,
                             float* out_nchw_or_null, void* stream);
/* label maps of the key sweep: transform.py:285-292 (undistortion), depth_transform :386-396 (T.Resize -- bilinear, for the
 * segmentation class ids too, as the reference does --, crop, flip); no normalisation.  maps f32 [B,N,H,W] (depth in metres
 * or class ids) -> out f32 [B,N,out_h,out_w].  One call per kind. */
int tt_preprocess_labels_ida(const float* maps, int B, int N, int H, int W, const float* mapx, const float* mapy,
                             const tt_ida_set* sets, int out_h, int out_w, float* out, void* stream);

/* ------------------------------------------------------------------------
 * The colour augmentation of training frames: ImageTransformMulti(aug=True) and its imgaug `augmenter(iteration)`
 * (datasets/pipelines/transform.py:142-216): a random-order sequence of eight operators on uint8 images (GaussianBlur,
 * AdditiveGaussianNoise, CoarseDropout, Dropout, Add, Multiply, LinearContrast, Grayscale), each under Sometimes(frequency),
 * made deterministic per sample, so all T x N frames of a sample get the same order, parameters and per-pixel random fields.
 *
 * The host (thinktwice_amd/photometric.py) draws one *program* per sample and compiles it into at most TT_AUG_MAX_OPS device
 * steps; the device only executes tables.  imgaug's random stream is not reproduced, and every rounding convention of
 * imgaug 0.4.0 / cv2 adopted here is UNPINNED (neither is installed where this was written): each lives in one host function
 * of photometric.py (INTEGRATION 2c lists them).  Step kinds, on integer grey levels v in 0..255 of pixel (y, x), channel c:
 *   LUT      v = lut[c][v]                                   (Add, Multiply, LinearContrast; adjacent ones composed on the host)
 *   NOISE    v = clip(v + k), k = -TT_AUG_NOISE_K + #{j : u >= cum[j]}: round(N(0, scale)) by its cumulative u32 thresholds
 *   DROPOUT  v = 0 where u < threshold
 *   COARSE   the same on the field value of cell (y * grid_h / H, x * grid_w / W) (integer division)
 *   GRAY     g = (4899 R + 9617 G + 1868 B + 8192) >> 14; v = clip(rint(f32(v) + alpha * f32(g - v)))
 *   BLUR     5 x 5 separable Gaussian, reflect-101 border, f32: horizontal then vertical, each summed
 *            ((((g0 p0 + g1 p1) + g2 p2) + g3 p3) + g4 p4) without fused multiply-add, then rint and clip; at most one per program
 * The field value u is the high 32 bits of splitmix64 at seed + 0x9E3779B97F4A7C15 * (idx + 1) (the mix of the dropout
 * kernel), idx = (c * H + y) * W + x when per_channel, else y * W + x shared by the channels; for COARSE idx runs over
 * the grid's cells the same way.  idx never depends on the image: every frame of a sample gets the same field.
 *
 * Programs are too large for kernel arguments: the caller keeps the B programs in host memory (checked by the entry before
 * any launch, the error naming the sample) and a copy in device memory (read by the kernels).  The entries do not copy,
 * allocate or synchronise.  A program with a BLUR needs `scratch`: tt_photometric_scratch_bytes(images, H, W) bytes (one packed
 * 4-byte pixel per pixel; the point steps before the blur write it, the blur kernel reads it).
 * ---------------------------------------------------------------------- */
#define TT_AUG_MAX_OPS 8
#define TT_AUG_NOISE_K 4
#define TT_AUG_LUT 0
#define TT_AUG_NOISE 1
#define TT_AUG_DROPOUT 2
#define TT_AUG_COARSE 3
#define TT_AUG_GRAY 4
#define TT_AUG_BLUR 5
typedef struct tt_aug_op {
    int kind;                            /* TT_AUG_* */
    int per_channel;                     /* NOISE, DROPOUT, COARSE: a field value per channel */
    int grid_h, grid_w;                  /* COARSE: cells, 1..H and 1..W */
    unsigned threshold;                  /* DROPOUT, COARSE: floor(p * 2^32) */
    float alpha;                         /* GRAY: 0..1 */
    unsigned long long seed;             /* NOISE, DROPOUT, COARSE: field seed */
    unsigned cum[2 * TT_AUG_NOISE_K];    /* NOISE: cum[j] = floor(2^32 * Phi((-K + j + 0.5) / scale)), non-decreasing */
    float taps[5];                       /* BLUR: normalised, >= 0 */
    int reserved;
    unsigned char lut[3][256];           /* LUT: one table per channel */
} tt_aug_op;                             /* 856 bytes */
typedef struct tt_aug_program {
    int num_ops;                         /* 0..TT_AUG_MAX_OPS */
    int blur_index;                      /* index of the BLUR step, -1 without one */
    tt_aug_op ops[TT_AUG_MAX_OPS];
} tt_aug_program;                        /* 6856 bytes */

/* Host arithmetic only: the scratch a call over `num_images` images of H x W needs when any program has a BLUR. */
long long tt_photometric_scratch_bytes(int num_images, int H, int W);
/* uint8 images that have been pre-processed already: in_u8 / out_u8 [B, per_sample, H, W, 3] (device; out may not alias in),
 * image (b, k) under program b. */
int tt_photometric_u8(const uint8_t* in_u8, int B, int per_sample, int H, int W, const tt_aug_program* programs_host,
                      const tt_aug_program* programs_dev, void* scratch, long long scratch_bytes, uint8_t* out_u8,
                      void* stream);
/* The fused path: tt_preprocess_images_ida's gather (same arguments, same checks), then what the reference does between the
 * two transforms and after: astype(uint8) -- (int)v truncation, clamped to 0..255 --, the program of the image's sample,
 * /255 and Normalize.  With all-empty programs it differs from tt_preprocess_images_ida by that truncation alone. */
int tt_preprocess_images_ida_aug(const uint8_t* raw_hwc, int B, int T, int N, int H, int W, const float* mapx,
                                 const float* mapy, const tt_ida_set* sets, int out_h, int out_w, const float* mean3,
                                 const float* std3, void* out_nhwc, int out_channels_padded, int out_dtype,
                                 float* out_nchw_or_null, const tt_aug_program* programs_host,
                                 const tt_aug_program* programs_dev, void* scratch, long long scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The two label inputs of the training image pipeline from the dataset's raw bytes: LoadDepth.__call__ and LoadSeg.__call__
 * with red_green_yellow (open_loop_training/code/datasets/pipelines/loading.py:84-93, :96-113, :132-162).  The PNG files are
 * decoded by tt_png_decode_u8 (below); union2one's meta merge stays on the host.  Everything but the depth quotient is integer
 * arithmetic: the outputs are bit-identical from run to run.
 * ---------------------------------------------------------------------- */
/* loading.py:88-90.  CARLA depth PNG pixels uint8 [n_pixels, 3] (R, G, B) -> metres f32 [n_pixels]:
 * f32(f32(code / 16777215.0f) * 1000.0f), code = R + 256 G + 65536 B (exact in f32), the division IEEE-rounded, nothing
 * contracted: the bits of the numpy float32 expression for every code. */
int tt_decode_depth_u8(const uint8_t* rgb_u8, long long n_pixels, float* out_f32, void* stream);

/* loading.py:97, cv2.cvtColor(..., COLOR_RGB2HSV) on uint8 (H in 0..179).  The device executes two division tables:
 *   v = max(R, G, B), diff = v - min(R, G, B), s = (diff * sdiv[v] + 2048) >> 12,
 *   h0 = G - B where v == R, else B - R + 2 diff where v == G, else R - G + 4 diff,
 *   h = (h0 * hdiv[diff] + 2048) >> 12 (arithmetic shift), plus 180 where negative.
 * The tables are the convention of OpenCV 4.x's integer path (RGB2HSV_b) and UNPINNED (cv2 is not installed where this was
 * written): thinktwice_amd/labels.py::hsv_tables is their one owner.  `tables` is a HOST pointer; the entry copies it into
 * the kernel's arguments (no device buffer, the caller may reuse the memory on return).  rgb_u8 / hsv_u8 uint8 [n_pixels, 3]. */
typedef struct tt_hsv_tables {
    int sdiv[256];                       /* rint(255 * 4096 / i), entry 0 is 0 */
    int hdiv[256];                       /* rint(180 * 4096 / (6 i)), entry 0 is 0 */
} tt_hsv_tables;                         /* 2048 bytes */
int tt_rgb2hsv_u8(const uint8_t* rgb_u8, long long n_pixels, const tt_hsv_tables* tables, uint8_t* hsv_u8, void* stream);

/* loading.py:132-162 with :96-113.  tags uint8 [num_samples, cams, H, W] (CARLA semantic tags) -> class ids f32 of that shape:
 *   - out = class_of_tag[tag] for every pixel whose tag is not light_tag (:159; a tag outside seg_label_idxs maps to 0);
 *   - the light_tag mask of every image is split into 8-connected components (:144).  A component of fewer than min_pixels
 *     pixels stays 0 (:153); every other one gets light_base + light_type (:157), light_type from the HSV values of its
 *     pixels in the image's RGB frame: sat_low = sat_low_of_avg[sum S / count] (integer division, :98-99), green = #{H in
 *     green_lo..green_hi, S >= sat_low, V >= val_low}, red likewise with red_lo..red_hi (:102-108); 0 where both < 3, 1 where
 *     red >= green, else 2 (:109-113).
 * rgb_u8: image (b, n) is the contiguous uint8 [H, W, 3] at rgb_u8 + b * rgb_sample_stride_bytes + n * H * W * 3, so the key
 * sweep raw[:, -1] of a contiguous [B, T, N, H, W, 3] tensor is read in place.  `conf` is a HOST pointer, copied into the
 * kernels' arguments.  `workspace`: tt_decode_seg_workspace_bytes(num_samples * cams, H, W) bytes, 8-byte aligned; the
 * kernels initialise every word they read, its contents on entry never matter.
 * Phases, one launch each, no workgroup ever waits for another: tile-local label equivalence in LDS (with the class map);
 * unions across tile edges and corners; flattening to roots; count and sum of S per root; green / red counts per root; the
 * write.  Labels are pixel indices within the image and only ever decrease.  Without a light tag only the first runs.
 * Returns an error before any launch for a null pointer, a non-positive size, H * W beyond int32, a short or misaligned
 * workspace, a light_tag outside -1..255 or a light class outside 0..253. */
typedef struct tt_seg_decode_conf {
    unsigned char class_of_tag[256];     /* position of the tag in seg_label_idxs, 0 for a tag that is not in it */
    int light_tag;                       /* the traffic-light tag (18), -1 for none */
    int light_base;                      /* its position in seg_label_idxs */
    int min_pixels;                      /* 20 */
    int val_low;                         /* 140 */
    int green_lo, green_hi;              /* 70, 100 */
    int red_lo, red_hi;                  /* 150, 180 */
    int sat_low_of_avg[256];             /* int(avg * 1.1), filled on the host with the reference's own expression */
    tt_hsv_tables hsv;
} tt_seg_decode_conf;                    /* 3360 bytes */
/* Host arithmetic only; 0 for a non-positive argument. */
long long tt_decode_seg_workspace_bytes(long long num_images, int H, int W);
int tt_decode_seg_u8(const uint8_t* tags_u8, int num_samples, int cams, int H, int W, const uint8_t* rgb_u8,
                     long long rgb_sample_stride_bytes, const tt_seg_decode_conf* conf, void* workspace,
                     long long workspace_bytes, float* out_f32, void* stream);
/* Measurement only (thinktwice_amd/bench_labels.py times the phases by difference): the same call cut short after phase
 * `last_phase`, 0 tile .. 5 write; only 5 leaves a complete output. */
int tt_decode_seg_u8_phases(const uint8_t* tags_u8, int num_samples, int cams, int H, int W, const uint8_t* rgb_u8,
                            long long rgb_sample_stride_bytes, const tt_seg_decode_conf* conf, void* workspace,
                            long long workspace_bytes, float* out_f32, int last_phase, void* stream);

/* ------------------------------------------------------------------------
 * The dataset's PNG files decoded on the device: what `np.array(Image.open(...))` returns for the camera frames, the depth
 * maps and the segmentation maps (open_loop_training/code/datasets/pipelines/loading.py:40-49, :127-131), from the files'
 * zlib streams.  The files are PIL's (`Image.fromarray(a).save(path)`): 8-bit, non-interlaced, colour type 2 (RGB) or 0
 * (grey), one zlib stream over the IDAT chunks, a filter type per row.  The decoder is specified for that family: chunk
 * walking is the caller's (thinktwice_amd/png.py::parse_png); the device gets the concatenated IDAT payload.
 *
 * One call decodes `num_images` images in two stream-ordered launches, nothing between them on the host:
 *   inflate   one 64-lane workgroup per image: RFC 1950 wrapper (CM = 8, window <= 32 KiB, no preset dictionary), RFC 1951
 *             stored, fixed and dynamic blocks -> the filtered scanlines, H * (1 + W * C) bytes, in the workspace.  The window
 *             is a 32 KiB ring in LDS; a match of any overlap gives byte i = out[pos - dist + (i mod dist)].
 *   unfilter  one 64-lane workgroup per image, 64 consecutive rows as a skewed wavefront (PNG specification section 9:
 *             None, Sub, Up, Average, Paeth) -> uint8 [H, W, C] at out_base + dst_offset, the filter bytes dropped.
 * Layouts.  packed_dev: one device buffer, 16-byte aligned, that holds every stream (and may hold images_dev); image i's
 * stream is its bytes [stream_offset, stream_offset + stream_bytes).  The table lives in host memory (images_host, validated
 * by the entry before any launch) and in device memory (images_dev, read by the kernels): it is past what kernel arguments
 * hold.  dst_offset lets one call fill slots of several tensors (raw[b, t, n], depth[b, n], seg[b, n]): offsets are relative
 * to out_base, destinations may lie in any order and must not overlap.  workspace: tt_png_workspace_bytes(...) bytes, 256-byte
 * aligned; image i's scanlines start at the sum of the earlier images' sizes, each rounded up to 256.  Its contents on entry
 * never matter.  status_dev: int32 [num_images], written by the kernels: TT_PNG_OK or the first error of the image.  An
 * image with an error leaves its destination untouched and does not affect the others.
 * NOT checked: the Adler-32 trailer of the zlib stream (its four bytes must be present, their value is not read), and
 * nothing of the PNG container (chunk CRC-32s are the host parser's, optional there): tt_png_decode_u8_verified, below,
 * checks both on the device.
 * Returns an error before any launch for: a null pointer; num_images < 1 or > TT_PNG_MAX_IMAGES; channels not 1 or 3; a
 * non-positive width or height; width > TT_PNG_MAX_WIDTH; H * (1 + W * C) above 2^31 - 1; a stream range outside
 * packed_bytes, shorter than 6 bytes or longer than 2^31 - 17; a destination range outside out_bytes; destinations that
 * overlap; a packed buffer or workspace that is misaligned; a workspace that is too small.  No allocation, no copy, no
 * synchronisation.
 * ---------------------------------------------------------------------- */
#define TT_PNG_MAX_IMAGES 1024
#define TT_PNG_MAX_WIDTH 8192            /* pixels per row: the unfilter keeps one row of packed pixels in LDS */
enum tt_png_status {
    TT_PNG_OK = 0,
    TT_PNG_TRUNCATED = 1,                /* the stream ends inside a header, a code, extra bits, stored bytes or the Adler-32 */
    TT_PNG_BAD_ZLIB_HEADER = 2,          /* CM != 8, window > 32 KiB, FCHECK, or a preset dictionary */
    TT_PNG_BAD_BLOCK_TYPE = 3,           /* BTYPE 3; inside a segment (tt_png_decode_u8_segmented), a block with BFINAL set */
    TT_PNG_BAD_STORED_LEN = 4,           /* LEN != ~NLEN */
    TT_PNG_BAD_CODE_LENGTHS = 5,         /* over-subscribed or unacceptably incomplete code, a repeat with no previous length,
                                            a run past the last code, HLIT > 286, HDIST > 30, no end-of-block code */
    TT_PNG_BAD_SYMBOL = 6,               /* a bit pattern no code has; length symbol 286 / 287, distance symbol 30 / 31 */
    TT_PNG_BAD_DISTANCE = 7,             /* a distance before the first output byte (of a segment: ITS first byte) or beyond the
                                            stream's window */
    TT_PNG_OUTPUT_OVERRUN = 8,           /* more than H * (1 + W * C) bytes */
    TT_PNG_OUTPUT_SHORT = 9,             /* fewer */
    TT_PNG_BAD_FILTER = 10               /* a row's filter type above 4 */
};
typedef struct tt_png_image {
    long long stream_offset;             /* of the zlib stream in packed_dev, bytes */
    long long stream_bytes;              /* >= 6 */
    long long dst_offset;                /* of the image's uint8 [H, W, C] in out_base, bytes */
    int width, height;
    int channels;                        /* 1 (grey) or 3 (RGB) */
    int reserved;                        /* not read */
} tt_png_image;                          /* 40 bytes */
/* Host arithmetic only; 0 for a null table, a bad count or an image the entry would refuse for its sizes. */
long long tt_png_workspace_bytes(const tt_png_image* images_host, int num_images);
int tt_png_decode_u8(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                     const tt_png_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                     uint8_t* out_base, long long out_bytes, int32_t* status_dev, void* stream);
/* Measurement only (thinktwice_amd/bench_png.py): the same call with only the inflate launch (phases = 1) or both (2). */
int tt_png_decode_u8_phases(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                            const tt_png_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                            uint8_t* out_base, long long out_bytes, int32_t* status_dev, int phases, void* stream);

/* ------------------------------------------------------------------------
 * Checksums of byte ranges of one device buffer: what `zlib.adler32(data, value)` (kind TT_CHECKSUM_ADLER32) and
 * `zlib.crc32(data, value)` (TT_CHECKSUM_CRC32) return for data = data_dev[offset, offset + bytes), bit for bit.
 * ranges: a table of num_ranges entries, in host memory (validated by the entry before any launch) and in device memory
 * (read by the kernels), the same contents.  Ranges may have any length including 0, start at any byte, lie in any order,
 * touch or overlap.  start_dev_or_null: uint32 [num_ranges], the running value of each range (zlib's second argument); null
 * means 1 for Adler-32 and 0 for CRC-32.  out_dev: uint32 [num_ranges].
 * Three stream-ordered launches (csrc/checksum.hip, csrc/png_checksum.h): a range is cut into tiles of TT_CHECKSUM_TILE bytes,
 * one 256-lane workgroup per tile, each lane a contiguous slice; one lane per range then folds the range's tiles in order and
 * applies the start value.  workspace: tt_checksum_workspace_bytes(...) bytes, 256-byte aligned, contents irrelevant.
 * Returns an error before any launch for: a null pointer (start excepted); num_ranges < 1 or > TT_CHECKSUM_MAX_RANGES; a
 * negative `bytes`; a range outside [0, data_bytes); an unknown kind; more than 2^31 - 1 tiles; a misaligned table, start,
 * output or workspace; a workspace that is too small.  No allocation, no copy, no synchronisation.
 * ---------------------------------------------------------------------- */
#define TT_CHECKSUM_TILE 65536           /* bytes per workgroup: the IDAT chunk size PIL writes */
#define TT_CHECKSUM_MAX_RANGES 1048576
enum tt_checksum_kind {
    TT_CHECKSUM_ADLER32 = 0,
    TT_CHECKSUM_CRC32 = 1
};
typedef struct tt_checksum_range {
    long long offset;                    /* of the range's first byte in data_dev */
    long long bytes;                     /* >= 0 */
} tt_checksum_range;                     /* 16 bytes */
/* Host arithmetic only; 0 for a null table, a bad count, a negative length or more than 2^31 - 1 tiles. */
long long tt_checksum_workspace_bytes(const tt_checksum_range* ranges_host, int num_ranges);
int tt_checksum_ranges_u8(const uint8_t* data_dev, long long data_bytes, const tt_checksum_range* ranges_host,
                          const tt_checksum_range* ranges_dev, int num_ranges, int kind, const uint32_t* start_dev_or_null,
                          uint32_t* out_dev, void* workspace, long long workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * tt_png_decode_u8 with the files' checksums verified on the device, between the inflate and the unfilter:
 *   TT_PNGV_ADLER32  the zlib stream's Adler-32 (RFC 1950): the four big-endian bytes that follow the final block's padding
 *                    to a byte boundary (NOT the stream's last four bytes: bytes after the trailer are accepted, as before)
 *                    against zlib.adler32 of the H * (1 + W * C) scanline bytes the inflate wrote.  This is what PIL and
 *                    zlib.decompress check ("incorrect data check"); the plain entry accepts such a stream.
 *   TT_PNGV_CRC32    every IDAT chunk's CRC-32 field against zlib.crc32(body, zlib.crc32(b"IDAT")) of its body in packed_dev.
 *                    Beyond PIL, which accepts an IDAT chunk with a wrong CRC field.
 * verify_flags is an OR of the two; 0 gives the bytes and statuses of tt_png_decode_u8 (the tables may then be null).
 * chunks (host and device copy, as the image table): one entry per IDAT chunk, the chunks of image 0 first, then image 1's,
 * ...; an image's chunks must tile its stream [stream_offset, stream_offset + stream_bytes) exactly and in order (a chunk
 * may be empty, and may start at any byte).  Only read with TT_PNGV_CRC32.
 * Status of an image, first match: the inflate's own error; TT_PNGV_BAD_CRC32 if any of its chunks fails; TT_PNGV_BAD_ADLER32;
 * the unfilter's TT_PNG_BAD_FILTER.  The two codes continue enum tt_png_status (11, 12) under a prefix of their own: only this
 * entry returns them.  As with every other status, a failed image's destination is untouched.
 * Launches: the tile plan, the inflate (which also hands out each stream's trailer), the checksum tiles over every image's
 * scanlines and every chunk, fold + compare + status (one lane per range), the unfilter.
 * workspace: tt_png_verify_workspace_bytes(...) bytes, 256-byte aligned; it begins with tt_png_decode_u8's workspace.
 * Returns an error before any launch for everything tt_png_decode_u8 refuses, and for: unknown flag bits; a null chunk table
 * or num_chunks < 1 with TT_PNGV_CRC32; num_chunks > TT_PNG_MAX_CHUNKS; a chunk whose image is out of range or below the
 * previous chunk's; a negative chunk length; chunks that do not tile their image's stream; an image without chunks.
 * ---------------------------------------------------------------------- */
#define TT_PNG_MAX_CHUNKS 1000000
enum tt_png_verify {
    TT_PNGV_ADLER32 = 1,
    TT_PNGV_CRC32 = 2,
    TT_PNGV_BAD_ADLER32 = 11,            /* status: the scanlines' Adler-32 is not the stream's trailer */
    TT_PNGV_BAD_CRC32 = 12               /* status: an IDAT chunk's CRC-32 is not its CRC field */
};
typedef struct tt_png_chunk {
    long long offset;                    /* of the chunk's body in packed_dev, bytes */
    long long bytes;                     /* >= 0 */
    unsigned crc;                        /* the chunk's CRC field: over the type bytes "IDAT" and the body */
    int image;                           /* index into the image table */
} tt_png_chunk;                          /* 24 bytes */
/* Host arithmetic only; 0 where the entry would refuse the tables. */
long long tt_png_verify_workspace_bytes(const tt_png_image* images_host, int num_images, const tt_png_chunk* chunks_host,
                                        int num_chunks, int verify_flags);
int tt_png_decode_u8_verified(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                              const tt_png_image* images_dev, int num_images, const tt_png_chunk* chunks_host,
                              const tt_png_chunk* chunks_dev, int num_chunks, int verify_flags, void* workspace,
                              long long workspace_bytes, uint8_t* out_base, long long out_bytes, int32_t* status_dev, void* stream);

/* ------------------------------------------------------------------------
 * tt_png_decode_u8_verified for files whose zlib stream has restart points, every SEGMENT of a stream inflated by a wave of
 * its own.  A stream written with a full flush (Z_FULL_FLUSH) after every R rows is one valid zlib stream; at each flush point
 * it is byte-aligned, the block before it is an empty stored block (00 00 FF FF) and no later match reaches back across it.
 * thinktwice_amd/png.py::segment_png writes such files and records the cut points in a private ancillary chunk (`ttSG`);
 * read_segments reads them back.  This entry takes them as a table:
 *   segment  bytes [offset, offset + bytes) of packed_dev, inside its image's stream and past its two header bytes: whole
 *            non-final deflate blocks, the last of them an empty stored block, that inflate to the image's scanlines
 *            [first_row, first_row + rows).  An image's segments stand together in the table, in row order, tile [0, H) and
 *            follow each other in the stream without a gap; the images of the table are in increasing order.
 *   tail     what follows an image's last segment, to the end of its stream: one final block without output (03 00, or
 *            01 00 00 FF FF), then the four Adler-32 bytes, which are the trailer TT_PNGV_ADLER32 compares.
 * An image WITHOUT an entry in the table is decoded by one wave over its whole stream, as by tt_png_decode_u8_verified, in the
 * same launch; num_segments = 0 (the segment tables may then be null) gives that entry's bytes and statuses.  The window of a segmented image is read from its
 * stream's CMF byte on the device and the header is checked as for a whole stream (TT_PNG_BAD_ZLIB_HEADER).
 * Launches: (the tile plan,) the inflate: one 64-lane workgroup per segment and one per image (its tail, or its whole
 * stream); the statuses' fold, one lane per image; then as tt_png_decode_u8_verified: checksum tiles, fold + compare, the
 * unfilter, all unchanged: they read the same workspace layout.  No workgroup waits for another.
 * A segment's scanlines start at first_row * (1 + W * C) of the image's slot, in general not 16-byte aligned; a wave stores
 * 16 bytes at a time only where the whole aligned group is its segment's, bytes at the two ends.
 * Status of an image, first match: the error of its LOWEST-NUMBERED failing segment (whatever the order the waves ran in);
 * its tail's error; then as tt_png_decode_u8_verified.  Inside a segment a block with BFINAL set is TT_PNG_BAD_BLOCK_TYPE, a
 * match that reaches before the segment's first byte TT_PNG_BAD_DISTANCE (so a stream cut at a sync flush, or an index that
 * does not fit its stream, ends in a status: no wave reads what another writes), rows that come out long or short
 * TT_PNG_OUTPUT_OVERRUN / TT_PNG_OUTPUT_SHORT, input that ends before the closing stored block TT_PNG_TRUNCATED.  A failed
 * image leaves its destination untouched and does not affect the others.
 * workspace: tt_png_segmented_workspace_bytes(...) bytes, 256-byte aligned; it begins with tt_png_decode_u8_verified's.
 * Returns an error before any launch for everything tt_png_decode_u8_verified refuses, and for: num_segments < 0 or
 * > TT_PNG_MAX_SEGMENTS; a null or misaligned segment table with num_segments > 0; an image index out of range or below the
 * previous entry's; an image's segments out of row order, with rows < 1, or not tiling [0, H); a segment that is empty,
 * does not start at its image's stream_offset + 2 or at the previous segment's end, or leaves fewer than 6 bytes of the
 * stream for the tail; a segmented image with more than 2^31 - 17 scanline bytes.
 * ---------------------------------------------------------------------- */
#define TT_PNG_MAX_SEGMENTS 1048576
typedef struct tt_png_segment {
    long long offset;                    /* of the segment's first byte in packed_dev */
    long long bytes;                     /* >= 1; a well-formed one has at least 5 and ends in 00 00 FF FF */
    int image;                           /* index into the image table */
    int first_row;
    int rows;                            /* >= 1 */
    int reserved;                        /* not read */
} tt_png_segment;                        /* 32 bytes */
/* Host arithmetic only; 0 where the entry would refuse the tables. */
long long tt_png_segmented_workspace_bytes(const tt_png_image* images_host, int num_images, const tt_png_chunk* chunks_host,
                                           int num_chunks, int verify_flags, const tt_png_segment* segments_host,
                                           int num_segments);
int tt_png_decode_u8_segmented(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                               const tt_png_image* images_dev, int num_images, const tt_png_chunk* chunks_host,
                               const tt_png_chunk* chunks_dev, int num_chunks, int verify_flags,
                               const tt_png_segment* segments_host, const tt_png_segment* segments_dev, int num_segments,
                               void* workspace, long long workspace_bytes, uint8_t* out_base, long long out_bytes,
                               int32_t* status_dev, void* stream);
/* Measurement only (thinktwice_amd/bench_png.py): the same call up to and including the inflate launch and the statuses' fold
 * (phases = 1), or all of it (2). */
int tt_png_decode_u8_segmented_phases(const uint8_t* packed_dev, long long packed_bytes, const tt_png_image* images_host,
                                      const tt_png_image* images_dev, int num_images, const tt_png_chunk* chunks_host,
                                      const tt_png_chunk* chunks_dev, int num_chunks, int verify_flags,
                                      const tt_png_segment* segments_host, const tt_png_segment* segments_dev, int num_segments,
                                      void* workspace, long long workspace_bytes, uint8_t* out_base, long long out_bytes,
                                      int32_t* status_dev, int phases, void* stream);

/* ------------------------------------------------------------------------
 * PNG files WRITTEN on the device: uint8 [H, W, C] images (C = 1 grey, 3 RGB) -> complete files, born segmented: signature,
 * IHDR, the `ttSG` index exactly as thinktwice_amd/png.py lays it out (version 1, rows_per_segment, ceil(H / R), n + 1
 * big-endian offsets into the IDAT payload, offsets[0] = 2), ONE IDAT chunk with the whole zlib stream (78 01; per R rows one
 * segment of non-final deflate blocks that ends in the empty stored block 00 00 FF FF and inflates alone; 03 00; the Adler-32
 * of the filtered scanlines), IEND; every chunk with its CRC-32.  tt_png_decode_u8_segmented reads them one wave per segment,
 * any PNG reader reads them as ordinary files.  The bytes are a function of the pixels and the table only
 * (csrc/png_deflate.h, which tools/png_encode_host_check.cpp runs on the host to the same bytes).
 * Launches, stream-ordered, nothing between them on the host: the filter pass (one 64-lane workgroup per row; PNG
 * specification sections 9 and 12.8) -> the filtered scanlines in the workspace; the deflate, one 64-lane workgroup per
 * segment, into per-segment worst-case slots of the workspace (dynamic Huffman blocks over an LZ77 parse, stored blocks where
 * those would not be smaller); one workgroup per image that sums the segment sizes and writes the offsets and the fixed
 * chunks; the copy that compacts the segments into the payload; the checksum tile plan, the Adler-32 tiles and fold, the
 * CRC-32 tiles and fold (csrc/checksum.hip's kernels over csrc/png_checksum.h), written in place.
 * images: the table, in host memory (validated before any launch) and in device memory (read by the kernels).  Image i's
 * pixels are pixels_dev[pixel_offset, + H * W * C); its file goes to files_dev[file_offset, ...), a slot of at least
 * tt_png_encode_bound(&image, 1) bytes, 4-byte aligned, of which the call writes exactly file_sizes_dev[i] bytes (every byte
 * of the slot beyond them, and everything between slots, stays as it was).  No device-side status: every size is bounded.
 * workspace: tt_png_encode_workspace_bytes(...) bytes, 256-byte aligned, contents irrelevant.
 * Returns an error before any launch for: a null pointer; a misaligned table (8 bytes), files_dev or file offset (4),
 * file_sizes_dev (8) or workspace (256); num_images < 1 or > TT_PNG_MAX_IMAGES; channels not 1 or 3; height or width < 1;
 * rows_per_segment < 1; an unknown filter mode; pixels outside pixel_bytes; a slot outside files_bytes, smaller than the
 * bound, or overlapping another; a workspace that is too small; a zlib stream that could pass 2^31 - 8 bytes.  No
 * allocation, no copy, no synchronisation.
 * ---------------------------------------------------------------------- */
enum tt_png_filter {                    /* (a prefix of their own: TT_PNG_* are the decoder's status codes) */
    TT_PNGE_FILTER_NONE = 0,
    TT_PNGE_FILTER_SUB = 1,
    TT_PNGE_FILTER_UP = 2,
    TT_PNGE_FILTER_AVG = 3,
    TT_PNGE_FILTER_PAETH = 4,             /* 0..4: that type for every row */
    TT_PNGE_FILTER_ADAPTIVE = 5           /* per row the type with the smallest sum of |residual as int8|, the lowest on a tie */
};
typedef struct tt_png_enc_image {
    long long pixel_offset;              /* of the image's uint8 [H, W, C] in pixels_dev, bytes */
    long long file_offset;               /* of the image's slot in files_dev, bytes; a multiple of 4 */
    long long file_capacity;             /* bytes of the slot, >= tt_png_encode_bound of this image */
    int width, height;
    int channels;                        /* 1 (grey) or 3 (RGB) */
    int rows_per_segment;                /* >= 1 */
    int filter;                          /* enum tt_png_filter */
    int reserved;                        /* not read */
} tt_png_enc_image;                      /* 48 bytes */
/* Host arithmetic only.  The bound: the sum over the images of the largest file each can become (every segment stored);
 * both: 0 for a null table, a bad count or an image the entry would refuse for its sizes. */
long long tt_png_encode_bound(const tt_png_enc_image* images_host, int num_images);
long long tt_png_encode_workspace_bytes(const tt_png_enc_image* images_host, int num_images);
int tt_png_encode_u8(const uint8_t* pixels_dev, long long pixel_bytes, const tt_png_enc_image* images_host,
                     const tt_png_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                     uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, void* stream);
/* Measurement only (thinktwice_amd/bench_png_encode.py): the same call up to and including the filter pass (phases = 1), the
 * deflate (2), or all of it (3). */
int tt_png_encode_u8_phases(const uint8_t* pixels_dev, long long pixel_bytes, const tt_png_enc_image* images_host,
                            const tt_png_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                            uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, int phases, void* stream);

/* ------------------------------------------------------------------------
 * JPEG files WRITTEN on the device: uint8 [H, W, C] images (C = 1 grey, 3 RGB) -> complete baseline sequential DCT files
 * (ITU-T T.81, SOF0, 8-bit) in a JFIF wrapper, for any reader: SOI, APP0 "JFIF" 1.01 density 1:1, DQT, SOF0, DHT, DRI, SOS,
 * the scan, EOI.  Quantisation tables: Annex K scaled by `quality` (s = 5000 / q below 50, else 200 - 2 q; entry =
 * clamp((base * s + 50) / 100, 1, 255)).  Huffman tables: the four typical tables of Annex K.3, fixed: one pass over the image.
 * The arithmetic is integer and this project's own (csrc/jpeg_core.h states it): the files are NOT byte-equal to another
 * encoder's, they are a function of the pixels and the table only, and tools/jpeg_encode_host_check.cpp runs the same text on
 * the host to the same bytes.  A restart interval is restart_rows MCU rows (an MCU is 8 x 8 pixels, 16 x 16 at 4:2:0), so the
 * DRI value is restart_rows * ceil(W / MCU width); an interval's scan bytes depend on its own blocks only.
 * Launches, stream-ordered, nothing between them on the host: the transform (one lane per 8 x 8 block: colour conversion,
 * chroma mean, DCT, quantisation -> int16 coefficients in zig-zag order, blocks in scan order, in the workspace); the entropy
 * pass, one 64-lane workgroup per restart interval, into per-interval worst-case slots of the workspace; one lane per image
 * that sums the interval sizes and writes the headers and file_sizes_dev[i]; the copy that compacts the intervals into the file.
 * images: the table, in host memory (validated before any launch) and in device memory (read by the kernels).  Image i's
 * pixels are pixels_dev[pixel_offset, + H * W * C); its file goes to files_dev[file_offset, ...), a slot of at least
 * tt_jpeg_encode_bound(&image, 1) bytes, 4-byte aligned, of which the call writes exactly file_sizes_dev[i] bytes (every byte
 * of the slot beyond them, and everything between slots, stays as it was).  No device-side status: every size is bounded
 * (a coefficient is at most 16 + 11 bits, 64 per block, every byte may be stuffed, a marker per interval, the fixed header).
 * workspace: tt_jpeg_encode_workspace_bytes(...) bytes, 256-byte aligned, contents irrelevant.
 * Returns an error before any launch for: a null pointer; a misaligned table (8 bytes), files_dev or file offset (4),
 * file_sizes_dev (8) or workspace (256); num_images < 1 or > TT_PNG_MAX_IMAGES; channels not 1 or 3; height or width outside
 * 1..65535; quality outside 1..100; an unknown subsampling; restart_rows < 1 or a DRI value above 65535; pixels outside
 * pixel_bytes; a slot outside files_bytes, smaller than the bound, or overlapping another; a workspace that is too small.  No
 * allocation, no copy, no synchronisation.
 * ---------------------------------------------------------------------- */
enum tt_jpeg_subsampling {
    TT_JPEG_444 = 0,                     /* every component at full size */
    TT_JPEG_420 = 1                      /* Cb and Cr at half size in both directions; grey images ignore it */
};
typedef struct tt_jpeg_enc_image {
    long long pixel_offset;              /* of the image's uint8 [H, W, C] in pixels_dev, bytes */
    long long file_offset;               /* of the image's slot in files_dev, bytes; a multiple of 4 */
    long long file_capacity;             /* bytes of the slot, >= tt_jpeg_encode_bound of this image */
    int width, height;                   /* 1..65535 */
    int channels;                        /* 1 (grey) or 3 (RGB) */
    int quality;                         /* 1..100 */
    int subsampling;                     /* enum tt_jpeg_subsampling */
    int restart_rows;                    /* >= 1: MCU rows per restart interval */
    int reserved;                        /* not read */
    int reserved2;                       /* not read */
} tt_jpeg_enc_image;                     /* 56 bytes */
/* Host arithmetic only.  The bound: the sum over the images of the largest file each can become; both: 0 for a null table, a
 * bad count or an image the entry would refuse for its sizes or parameters. */
long long tt_jpeg_encode_bound(const tt_jpeg_enc_image* images_host, int num_images);
long long tt_jpeg_encode_workspace_bytes(const tt_jpeg_enc_image* images_host, int num_images);
int tt_jpeg_encode_u8(const uint8_t* pixels_dev, long long pixel_bytes, const tt_jpeg_enc_image* images_host,
                      const tt_jpeg_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                      uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, void* stream);
/* Measurement only (thinktwice_amd/bench_jpeg_encode.py): the same call up to and including the transform (phases = 1), the
 * entropy pass (2), or all of it (3). */
int tt_jpeg_encode_u8_phases(const uint8_t* pixels_dev, long long pixel_bytes, const tt_jpeg_enc_image* images_host,
                             const tt_jpeg_enc_image* images_dev, int num_images, void* workspace, long long workspace_bytes,
                             uint8_t* files_dev, long long files_bytes, long long* file_sizes_dev, int phases, void* stream);

/* ------------------------------------------------------------------------
 * Debug frames DRAWN on the device (thinktwice_amd/render.py, csrc/render.hip, csrc/render_raster.h): a caller-owned uint8 canvas
 * [Hc][Wc][3] filled from a display list, so that what the model predicted reaches tt_png_encode_u8 without a copy to the host.
 * The palette, look-up tables, layout and 5 x 7 font are this project's own (the reference draws nothing).
 *
 * The list is a table of tt_render_item, given in host memory (validated before any launch) and in device memory (read by the
 * kernels), drawn in painter's order by index, later over earlier.  The rasteriser is a GATHER: every canvas pixel starts black,
 * walks the items that can touch it and keeps the last word, so the picture is a function of the list and its sources only, not
 * of the launch geometry.  One 256-lane workgroup per tile of 8 rows x 256 columns; the list is staged through LDS in chunks of
 * TT_RENDER_CHUNK items (polyline points go to fixed point there, once per workgroup) and an item whose bounding box misses the
 * tile is skipped per workgroup.  EVERY byte of the canvas is written; nothing outside it is.
 * All arithmetic is integer, or f32 with every operation rounded separately (no contraction); csrc/render_raster.h holds the
 * per-pixel rules as __host__ __device__ functions, which tools/render_host_check.cpp compiles for the host.
 * Blend, everywhere: (dst * (256 - a) + src * a + 128) >> 8 per channel, weight a in 0..256.
 * An item is clipped to the canvas and to its own rectangle [x0, x0 + w) x [y0, y0 + h), which may lie partly or wholly outside
 * the canvas; w == 0 or h == 0 draws nothing.  `color` is r | g << 8 | b << 16.
 *
 *  FILL         the rectangle in `color` at weight `alpha`.
 *  IMAGE_F32    src: planar f32 [3][sh][sw] (a network input); pixel (x, y) of the rectangle shows source (x / scale, y / scale),
 *               channel c as clamp(rint(v * m[c] + m[3 + c]), 0, 255) in f32 in that order (m[0..3) = 255 std, m[3..6) = 255 mean: the
 *               inverse of tt_preprocess_images' normalisation of pixel / 255).  A NaN in any channel: `color`.  Weight `alpha`.
 *  IMAGE_U8     src: uint8 [sh][sw][channels] (1 or 3), reduced by the box factor `scale` >= 1: per channel
 *               (sum of scale x scale + scale * scale / 2) / (scale * scale).  Weight `alpha`.
 *  SEG_OVERLAY  src: f32 logits [sh][sw][stride >= channels] channel-last; the cell of pixel (x, y) is (x / scale, y / scale);
 *               argmax over [0, channels), ties to the lowest index, padding channels never read (tt_eval_seg_confusion's rule);
 *               aux: palette, channels x 4 bytes r, g, b, a, blended at weight a + (a >> 7) (0 leaves the pixel alone, 255 is
 *               opaque).  A NaN among the cell's `channels` logits: `color` at full weight.  channels <= 32.
 *  DEPTH_MAP    src: f32 logits [sh][sw][stride >= channels]; argmax bin, ties to the lowest (tt_eval_depth_bins' rule); colour
 *               aux[3 * (bin * 255 / (channels - 1))] of a 256 x 3 byte table (index 0 for one channel); nearest upscale by `scale`;
 *               a NaN: `color`.  Weight `alpha`.  channels <= 256.
 *  POINTS_BEV   src: f32 cloud [count][stride >= 3]; m: x, y metres -> 1/16-pixel units of the CANVAS, u = m0 x + m1 y + m2,
 *               v = m3 x + m4 y + m5.  The point's pixel is (floor(u) >> 4, floor(v) >> 4); its height index
 *               clamp(floor((z - p[0]) * p[1]), 0, 255).  The highest point of a pixel wins (an integer atomic maximum of
 *               index + 1 on the item's u32 scratch plane, h x w words at workspace + ws_offset) and is shown as aux[3 * index] of
 *               a 256 x 3 byte table at weight `alpha`.  Not drawn: a row with x = y = z = 0 (collate padding), a row with a
 *               non-finite x, y or z, a point beyond +-2^20 units or outside the rectangle or the canvas.
 *  POLYLINE_DEV src: f32 [count][2] DEVICE points (count <= TT_RENDER_MAX_POINTS), through a matrix m as above, each coordinate
 *               to fixed point by rint.  A pixel, by its centre (16 px + 8, 16 py + 8), belongs to a point's disc if
 *               dx^2 + dy^2 <= radius^2 (radius > 0) and to the segment of two consecutive points if its squared distance to
 *               the segment is <= half_width^2, in exact integer arithmetic (so A->B and B->A cover the same pixels, and a
 *               segment with equal endpoints is the disc of radius half_width).  Covered pixels take `color` at weight `alpha`.
 *               A point that is not finite, or beyond +-2^20 units after the matrix, is dropped with its segments, never
 *               converted to an integer, and adds 1 to status word TT_RENDER_STATUS_DROPPED.
 *  MARKER       the same from host floats p = (cx, cy, hx, hy) metres: count = TT_RENDER_MARKER_CROSS (the segments
 *               (cx - hx, cy)-(cx + hx, cy) and (cx, cy - hy)-(cx, cy + hy)) or TT_RENDER_MARKER_BOX (the closed loop of
 *               the four corners), sums and differences in f32.
 *  TEXT         src: `count` bytes; aux: the font, 256 bytes (character -> glyph number) then 8 bytes per glyph (7 rows, bit 4 =
 *               the leftmost of 5 columns); character i fills the cell of 6 x 8 font pixels of `scale` x `scale` canvas pixels
 *               at x0 + 6 i scale.  Set pixels take `color` at weight `alpha`.
 *
 * workspace: tt_render_workspace_bytes(...) bytes, 256-byte aligned: TT_RENDER_STATUS_WORDS int64 status words, then the scratch
 * planes; an item's ws_offset is that of its plane (a multiple of 256, planes in list order, none overlapping).  The caller zeroes
 * the workspace ONCE.  The status words are only ever added to; the caller reads and clears them when it wants them.  Every
 * scratch word the splat sets lies under a canvas pixel of its item, and the compose pass, which reads it exactly once, stores 0
 * back: the planes are all zero again when the call's last launch ends -- cleared by the pass that reads them, no memset.
 * Launches, stream-ordered: one splat per POINTS_BEV item with count > 0; one that counts dropped points when the list holds a
 * POLYLINE_DEV or MARKER; the compose.
 * Returns an error before any launch for: a null canvas, table or workspace, a null src / aux an item needs; a misaligned
 * device table (16 bytes) or workspace (256); a canvas side outside 1..16384; num_items < 0 or > TT_RENDER_MAX_ITEMS (no
 * truncation); an unknown kind; a negative w, h, count or a side above 16384; scale < 1; alpha outside 0..256; a rectangle larger
 * than its source gives (w > sw * scale, w > sw / scale for IMAGE_U8, w > 6 count scale for TEXT, likewise h); channels or
 * stride out of range; a negative radius or half_width, or one above 2^15; a non-finite m or p; a plane outside the workspace,
 * misplaced or overlapping.  No allocation, no copy, no synchronisation.
 * ---------------------------------------------------------------------- */
#define TT_RENDER_MAX_ITEMS 1024
#define TT_RENDER_CHUNK 32                 /* items per LDS stage */
#define TT_RENDER_MAX_POINTS 16            /* of one POLYLINE_DEV */
#define TT_RENDER_STATUS_WORDS 4           /* int64 each, at the start of the workspace */
#define TT_RENDER_STATUS_DROPPED 0
enum tt_render_kind {
    TT_RENDER_FILL = 0,
    TT_RENDER_IMAGE_F32 = 1,
    TT_RENDER_IMAGE_U8 = 2,
    TT_RENDER_SEG_OVERLAY = 3,
    TT_RENDER_DEPTH_MAP = 4,
    TT_RENDER_POINTS_BEV = 5,
    TT_RENDER_POLYLINE_DEV = 6,
    TT_RENDER_MARKER = 7,
    TT_RENDER_TEXT = 8,
    TT_RENDER_NUM_KINDS = 9
};
enum tt_render_marker {
    TT_RENDER_MARKER_CROSS = 0,
    TT_RENDER_MARKER_BOX = 1
};
typedef struct tt_render_item {
    int kind;                            /* enum tt_render_kind */
    int x0, y0, w, h;                    /* the item's own rectangle on the canvas, pixels */
    int sw, sh;                          /* the source's width and height: pixels or cells */
    int scale;                           /* upscale k, box factor s, seg factor f or text scale; >= 1 */
    int channels;                        /* IMAGE_U8: 1 or 3; SEG_OVERLAY: classes; DEPTH_MAP: bins */
    int stride;                          /* SEG_OVERLAY / DEPTH_MAP: floats per cell; POINTS_BEV: floats per row */
    int count;                           /* points, characters, or enum tt_render_marker */
    int alpha;                           /* 0..256 */
    unsigned color;                      /* r | g << 8 | b << 16 */
    int half_width, radius;              /* 1/16 pixel */
    int reserved;                        /* not read */
    float m[6];                          /* 2 x 3 matrix, or std[3] then mean[3] */
    float p[4];                          /* MARKER: cx, cy, hx, hy; POINTS_BEV: z_lo, inv_step */
    long long ws_offset;                 /* POINTS_BEV: bytes from the workspace to the item's scratch plane */
    const void* src;                     /* device */
    const void* aux;                     /* device */
} tt_render_item;                        /* 128 bytes */
/* Host arithmetic only: the status words plus, per POINTS_BEV item in list order, its plane rounded up to 256 bytes; 0 for a
 * null table with num_items > 0, a bad count or a rectangle the entry would refuse. */
long long tt_render_workspace_bytes(const tt_render_item* items_host, int num_items);
int tt_render_u8(uint8_t* canvas_dev, int Hc, int Wc, const tt_render_item* items_host, const tt_render_item* items_dev,
                 int num_items, void* workspace, long long workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * SURVEY 8f-4 (training step), optimizer half: the reference's `optimizer_config = dict(grad_clip=dict(max_norm=100,
 * norm_type=2))` and `optimizer = dict(type='AdamW', lr=1e-4, weight_decay=1e-7)` (configs/thinktwice.py:282-287:
 * torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW through mmcv's OptimizerHook) over ONE flat f32 parameter /
 * gradient buffer.  No host synchronisation: the clip coefficient stays on the device.
 * ---------------------------------------------------------------------- */
/* out_norm_scale[0] = ||grad||_2, [1] = min(1, max_norm / (norm + 1e-6)); workspace_1024: 1024 floats */
int tt_grad_norm_clip(const float* grad, long long n, float max_norm, float* workspace_1024,
                      float* out_norm_scale, void* stream);
/* one AdamW update of `n` parameters in place (p, exp_avg, exp_avg_sq); `step` >= 1 is the 1-based step count of
 * the bias correction; the gradient is multiplied by *grad_scale_or_null (device scalar, e.g. out_norm_scale + 1) */
int tt_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step,
                  const float* grad_scale_or_null, void* stream);
/* The same update with the step count ON THE DEVICE: the bias corrections use *good_steps_dev + 1; tt_adamw_advance, issued once
 * after the launches of one optimizer step, increments the count unless the clip factor is NaN (non-finite gradient norm: the
 * update was skipped, and the count stays with the moments whatever the host does meanwhile). */
int tt_adamw_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                      float beta1, float beta2, float eps, float weight_decay, const int* good_steps_dev,
                      const float* grad_scale_or_null, void* stream);
int tt_adamw_advance(int* good_steps_dev, const float* grad_scale_or_null, void* stream);
/* tt_adamw_advance for the close of a gradient-accumulation window of `window_len` >= 1 micro-iterations (Trainer.step(window=)):
 * the count advances unless the clip factor is NaN; then *skipped_iters_dev += window_len instead, so that the host can take a
 * skipped window's micro-iterations back out of its counters whatever the window's length was (Trainer.reconcile). */
int tt_adamw_advance_window(int* good_steps_dev, int* skipped_iters_dev, int window_len, const float* grad_scale_or_null,
                            void* stream);

/* ------------------------------------------------------------------------
 * Device log windows (thinktwice_amd/logvars.py): the logged values of a training job stay on the device from the loss terms to
 * the closed window, so the loop around Trainer.step never waits for them.
 *
 * tt_logvars_pack restates EncoderDecoder._parse_losses (encoder_decoder_framework.py:409-439) for one-element f32 terms, one
 * launch: packed[s] for every slot s (log name, dict order), packed[n_slots] = the total loss.  A slot is the sequential f32 sum
 * of its terms, in table order, starting from +0.0f: a plain entry has one term (`value.mean()` of one element is torch's
 * reduction from +0.0f, so -0.0 comes out as +0.0), a list entry several (`sum(v.mean() for v in value)`: Python's sum starts at
 * int 0).  The total is the sequential f32 sum, from +0.0f, in slot order, of the slots with in_loss[s] != 0 (the names containing
 * 'loss').  One thread does every sum, so the results are the bits of the torch expression, zeros' signs and NaN included.  The
 * table travels BY VALUE as the kernel argument: `terms` is a HOST pointer read during the call, nothing is uploaded.
 * ---------------------------------------------------------------------- */
#define TT_LOGVARS_MAX_TERMS 64
typedef struct tt_logvars_terms {
    const float* term[TT_LOGVARS_MAX_TERMS];         /* device f32 scalars, table order = dict order, list entries in list order */
    unsigned char slot[TT_LOGVARS_MAX_TERMS];        /* slot of term i, non-decreasing, every slot 0..n_slots-1 has >= 1 term */
    unsigned char in_loss[TT_LOGVARS_MAX_TERMS];     /* per slot */
} tt_logvars_terms;                                  /* 640 bytes */
/* 1 <= n_slots <= n_terms <= TT_LOGVARS_MAX_TERMS; packed: n_slots + 1 device floats */
int tt_logvars_pack(const tt_logvars_terms* terms, int n_terms, int n_slots, float* packed, void* stream);
/* One iteration into a window (eval_tool.py:96-109 `results[k] += v * batch_size`; mmcv LogBuffer.update).  `window`: n + n_tail
 * + 3 device doubles: the sums of packed[0..n) then tail[0..n_tail), then [total weight, iterations, skipped].  gate non-null and
 * gate[0] not finite: skipped += 1 and nothing else.  Otherwise sum[i] += (double)v[i] * weight, total weight += weight,
 * iterations += 1.  `tail` (nullable with n_tail == 0): a second f32 source vector.  0 < weight < 2^29; n >= 1; n + n_tail <= 1024.
 * Calls on one stream add in call order, in f64. */
int tt_logvars_accumulate(const float* packed, int n, const float* tail, int n_tail, int weight, const float* gate,
                          double* window, void* stream);
/* out[0..n_all) = window[0..n_all), then window[0..n_all) = 0, one launch (mmcv LogBuffer.average + clear_output: the division by
 * the total weight is the reader's).  `out` is DEVICE memory that does not overlap `window`; 1 <= n_all <= 1027. */
int tt_logvars_flush(double* window, int n_all, double* out, void* stream);

/* ------------------------------------------------------------------------
 * Open-loop task metrics on the device (thinktwice_amd/evaluate.py, csrc/eval_metrics.hip): a forward's heads against a loader
 * batch's labels, folded into caller-owned device accumulators.  Counts are int64 and added with integer atomics (exact, the
 * same bits every run); f64 sums are one workgroup's, in sample order; no entry waits for the host and calls on one stream
 * accumulate in call order.  The metric definitions are this project's; what is restated from the reference is which label a
 * cell is compared with.
 *
 * tt_eval_seg_confusion: logits_cl channel-last [BN][H/factor][W/factor][cstride >= num_classes], labels [BN][H][W] float class
 * ids -- the layout of tt_loss_seg_focal.  The label of cell (y, x) is the pixel (y*factor, x*factor): get_downsampled_gt_seg
 * (encoder_decoder_framework.py:485-491, torchvision's nearest resize).  The prediction is the argmax over channels
 * [0, num_classes), ties to the lowest index; padding channels take no part.  conf: num_classes * num_classes + 2 int64:
 * conf[label * num_classes + pred] += 1, then [bad_label, nonfinite].  Label 255 is skipped as in the loss; another label outside
 * [0, num_classes) adds to bad_label only; a cell whose num_classes logits hold a NaN adds to nonfinite only.
 * 1 <= num_classes <= 32; H and W divisible by factor.
 *
 * tt_eval_depth_bins: logits_cl [BN][H/factor][W/factor][cstride >= D], gt_depth [BN][H][W] metres (0 = no return) -- the layout
 * and the cell rule of tt_loss_depth_bce, i.e. get_downsampled_gt_depth (encoder_decoder_framework.py:443-482): g = min over the
 * factor x factor cell with 0 read as 1e5, (g - (d_lo - d_step)) / d_step in f32, outside [0, D + 1) -> 0, truncated: bin 0 is
 * background, bin k the depth channel k - 1.  acc: 5 int64 over the foreground cells: [n_fg, n_top1 (argmax == bin - 1, ties to
 * the lowest index), n_within1 (|argmax - (bin - 1)| <= 1), sum_abs_bins (the sum of that distance), nonfinite (a foreground
 * cell whose D logits hold a NaN: counted here and nowhere else)].
 *
 * tt_eval_decoder: pred_wp [B][S][4][2], mu_branches / sigma_branches [B][S][2], pred_speed [B] (the head's speed / 12,
 * encoder_decoder_framework.py:198) against the expert's waypoints [B][4][2], action_mu / action_sigma [B][2], speed [B] (m/s).
 * sums: 8 S + 1 doubles, per stage s at sums[8 s ..]: [ADE (mean over the 4 steps of the L2 distance), FDE (the last step's),
 * mean |dx| (longitudinal), mean |dy| (lateral), |mu - a_mu| columns 0 and 1, |sigma - a_sigma| columns 0 and 1], then
 * sums[8 S] = |12 pred_speed - speed|.  Every term is computed in f64 from the f32 inputs (differences, squares, their sum, sqrt,
 * the steps added in order, * 0.25) and every sum is ONE sequential f64 sum over the samples of all calls in order.  counts: 2
 * int64 [samples, nonfinite]: a sample with a non-finite pred_wp / mu / sigma / pred_speed value adds to nonfinite and to nothing
 * else.  1 <= S <= 7.
 *
 * tt_eval_pair_deviation: two f32 tensors of n elements (precision modes A and B of one output).  slots: 3 int64 [the bit
 * pattern of max |a - b| as f32, that of max |a|, the number of elements where a or b is not finite (they stay out of both
 * maxima)]; the maxima fold by integer maximum, which is exact for non-negative floats.
 * tt_eval_pair_wp: two pred_wp tensors of `points` (x, y) pairs: per pair the f64 L2 distance (what `(a - b).norm(dim=-1)`
 * measures).  max_sum: 2 doubles [maximum, sequential sum in index order]; counts: 2 int64 [finite points, others].
 * tt_eval_pair_seg: two seg logit maps [cells][cstride >= num_classes]: out: 3 int64 [cells whose argmax differs, cells compared,
 * cells with a NaN in either (not compared)].
 * ---------------------------------------------------------------------- */
int tt_eval_seg_confusion(const float* logits_cl, int cstride, int num_classes, const float* labels, int BN, int H, int W,
                          int factor, long long* conf, void* stream);
int tt_eval_depth_bins(const float* logits_cl, int cstride, int D, const float* gt_depth, int BN, int H, int W, int factor,
                       float d_lo, float d_step, long long* acc, void* stream);
int tt_eval_decoder(const float* pred_wp, const float* mu_branches, const float* sigma_branches, const float* pred_speed,
                    const float* waypoints, const float* action_mu, const float* action_sigma, const float* speed, int B, int S,
                    double* sums, long long* counts, void* stream);
int tt_eval_pair_deviation(const float* a, const float* b, long long n, long long* slots, void* stream);
int tt_eval_pair_wp(const float* a, const float* b, int points, double* max_sum, long long* counts, void* stream);
int tt_eval_pair_seg(const float* a_cl, const float* b_cl, int cstride, int num_classes, long long cells, long long* out,
                     void* stream);

/* ------------------------------------------------------------------------
 * SURVEY 8f-4, the torch-autograd route of the training step (thinktwice_amd/autograd_route.py): what mmcv's OptimizerHook gets
 * from `outputs['loss'].backward()` depositing into every parameter's `.grad` (apis/mmdet_train.py:70-97) -- here the reverse
 * sweep leaves one separately allocated f32 tensor per parameter, and ONE launch gathers `nseg` of them into one flat f32 buffer
 * (per-parameter views of which go back to autograd), scaled by the device scalar grad_output:
 *     flat[dst_off[i] .. + count[i])  (=|+=)  scale * src[i][0 .. count[i])
 * The work is cut by bytes (16 KiB pieces of the covered range, the segment(s) under a piece found by binary search), 16-byte
 * loads and stores where source and destination are co-aligned.  `scale * src` and the sum are rounded separately.  Elements
 * of `flat` no segment covers are not written.  nseg == 0: returns 0, launches nothing.
 * ---------------------------------------------------------------------- */
typedef struct tt_grad_seg {
    const void* src;        /* device f32 array of `count` elements, 4-byte aligned (may be a view inside a larger allocation) */
    long long dst_off;      /* first element of `flat` it lands on, >= 0; the table is sorted by it and the ranges do not overlap */
    long long count;        /* elements, >= 0 */
} tt_grad_seg;
/* segs_dev: the table in DEVICE memory (8-byte aligned); scale_dev_or_null: device scalar (null = 1.0); accumulate: 0 "=", 1 "+=" */
int tt_grad_gather(const tt_grad_seg* segs_dev, int nseg, float* flat, const float* scale_dev_or_null, int accumulate,
                   void* stream);

/* ----------------------------------------------------------------------
 * SURVEY 8f-4 / row A24, loss half of the training forward: device reductions for every term of
 * ThinkTwiceDecoder.loss (thinktwice_decoder.py:536-619), the focal segmentation loss (utils.py:31-47 at
 * encoder_decoder_framework.py:172-176) and the depth BCE (encoder_decoder_framework.py:179-190, 441-481).
 * One launch per term, f64 accumulation, workgroup partials combined in index order by the last workgroup
 * (bit-reproducible).  `workspace`: tt_loss_workspace_bytes() bytes, ZEROED once by the caller, reusable by
 * consecutive calls on one stream.  Outputs are device floats.
 * ---------------------------------------------------------------------- */
long long tt_loss_workspace_bytes(void);
/* pred [n_outer][repeat][inner] against target [n_outer][inner] (broadcast over `repeat`; NULL = zeros),
 * F.smooth_l1_loss(beta=1).  reduce != 0: out[0] = scale * mean(min(l, clamp_max)) (clamp_max <= 0: no clamp,
 * torch.clamp(..., -5, 5) of DEC:51-52 is clamp_max = 5); reduce == 0: out[i] = scale * l_i (reduction='none'). */
int tt_loss_smooth_l1(const float* pred, const float* target, long long n_outer, int repeat, long long inner,
                      float clamp_max, float scale, int reduce, float* out, void* workspace, void* stream);
/* gradients of the two mean-reduced decoder terms w.r.t. the prediction, dense in the prediction's layout (written, not
 * accumulated): dpred = d[scale * mean(...)]/dpred.  tt_loss_smooth_l1_bwd: zero where the clamp is active. */
int tt_loss_smooth_l1_bwd(const float* pred, const float* target, long long n_outer, int repeat, long long inner,
                          float clamp_max, float scale, float* dpred, void* stream);
int tt_loss_beta_kl_bwd(const float* target_alpha, const float* target_beta, const float* pred_alpha,
                        const float* pred_beta, long long n_outer, int repeat, long long inner, float scale,
                        float* dpred_alpha, float* dpred_beta, void* stream);
/* out[0] = scale * mean KL(Beta(target_alpha, target_beta) || Beta(pred_alpha, pred_beta)), target [n_outer][inner]
 * broadcast over pred [n_outer][repeat][inner] (torch.distributions.kl_divergence, DEC:553-556, 571-573) */
int tt_loss_beta_kl(const float* target_alpha, const float* target_beta, const float* pred_alpha,
                    const float* pred_beta, long long n_outer, int repeat, long long inner, float scale, float* out,
                    void* workspace, void* stream);
/* out[c] = mean_r |pred[r][c] - target[r][c]|, cols <= 8, pred rows pred_row_stride floats apart (DEC:544-551).
 * With pred_beta / target_beta non-NULL the operands are Beta parameters and their modes mapped to [-1, 1]
 * (_get_action_beta, DEC:622-637) are compared. */
int tt_loss_l1_cols(const float* pred, const float* pred_beta, long long pred_row_stride, const float* target,
                    const float* target_beta, long long rows, int cols, float* out, void* workspace, void* stream);
/* logits_cl: channel-last [BN][H/factor][W/factor][row_stride >= num_classes]; labels [BN][H][W] float class ids
 * (255 = ignore) sampled at (y*factor, x*factor); out[0] = 10 * focal(alpha .5, gamma 2) of the mean cross entropy;
 * out[1], out[2] = that mean cross entropy and the number of contributing pixels (`aux` of the backward): out holds 3 floats.
 * tt_loss_seg_focal_bwd: dlogits_cl = upstream (device scalar, NULL = 1) * d out[0] / d logits, padding channels 0. */
int tt_loss_seg_focal(const float* logits_cl, int row_stride, int num_classes, const float* labels, int BN, int H,
                      int W, int factor, float* out, void* workspace, void* stream);
int tt_loss_seg_focal_bwd(const float* logits_cl, int row_stride, int num_classes, const float* labels, int BN, int H,
                          int W, int factor, const float* aux, const float* upstream_or_null, float* dlogits_cl,
                          void* stream);
/* logits_cl: channel-last [BN][H/factor][W/factor][row_stride >= D]; gt_depth [BN][H][W] metres (0 = no return);
 * bins of d_step from d_lo; out[0] = sum of BCE-with-logits over the foreground cells / max(1, #foreground) */
int tt_loss_depth_bce(const float* logits_cl, int row_stride, int D, const float* gt_depth, int BN, int H, int W,
                      int factor, float d_lo, float d_step, float* out, void* workspace, void* stream);
/* out of tt_loss_depth_bce holds 2 floats (loss, divisor = `aux` here); dlogits_cl = upstream * d loss / d logits */
int tt_loss_depth_bce_bwd(const float* logits_cl, int row_stride, int D, const float* gt_depth, int BN, int H, int W,
                          int factor, float d_lo, float d_step, const float* aux, const float* upstream_or_null,
                          float* dlogits_cl, void* stream);

/* ----------------------------------------------------------------------
 * SURVEY 8f-4, backward of the convolution (what autograd + cuDNN do under loss.backward() in the reference,
 * apis/mmdet_train.py:72-79).  Weight gradient of tt_conv2d_fwd's channel-last convolution:
 *   dw[co][kh][kw][ci] (+)= sum_{n,oh,ow} dy[n][oh][ow][dy_coff + co] * x[n][oh*s - p + kh*d][ow*s - p + kw*d][x_coff + ci]
 * exact f32 products on the f32 MFMA, deterministic (split partial sums added in a fixed order).  dw has the weight
 * layout [Cout][KH][KW][cin_pad] (padding channels are written as 0).  The input gradient needs no entry of its own:
 * it is tt_conv2d_fwd of dy with the 180-degree-rotated, Cin/Cout-transposed weights (thinktwice_amd/ops.py::conv2d_dgrad).
 * ---------------------------------------------------------------------- */
long long tt_conv2d_wgrad_workspace_bytes(int N, int OH, int Cout, int Cin, int cin_pad, int KH, int KW);
int tt_conv2d_wgrad(const float* x, int N, int H, int W, int Cin, int x_cstride, int x_coff, const float* dy, int OH,
                    int OW, int Cout, int dy_cstride, int dy_coff, int KH, int KW, int stride, int pad, int dil,
                    int cin_pad, int accumulate, float* dw, void* workspace, long long workspace_bytes, void* stream);
/* Same contract in the forward's bf16x3 arithmetic (dy and x split into bf16 hi + lo, three MFMAs per product, f32
 * accumulation: ~2^-17 relative per product) on an LDS-staged v_mfma_f32_32x32x16_bf16 kernel (the contraction index -- the
 * pixel -- is the slow index of both operands: tiles of 32 pixels are staged as they lie in memory and read column-wise).
 * That kernel takes a layer with Cout >= 64 and Cin >= 64; Cout, Cin, x_cstride, x_coff, dy_cstride and dy_coff multiples of
 * 4; x and dy 16-byte aligned; and output rows of OW >= 16 pixels -- where a 1 x 1 / stride 1 / pad 0 layer with OW < 128
 * counts as regrouped into pseudo-rows of >= 128 pixels whenever its N * OH rows have a divisor that reaches them (a linear
 * layer over rows, OW = 1, qualifies from 128 rows on).  Every other layer runs tt_conv2d_wgrad's kernels in exact f32: a
 * routing decision, not an error.  Same workspace query (it is sized for tt_conv2d_wgrad's choice, and the row split of the
 * LDS-staged kernel is clamped to the slices it holds), same determinism.  All of it is csrc/wgrad_choose.cpp. */
int tt_conv2d_wgrad_x3(const float* x, int N, int H, int W, int Cin, int x_cstride, int x_coff, const float* dy, int OH,
                    int OW, int Cout, int dy_cstride, int dy_coff, int KH, int KW, int stride, int pad, int dil,
                    int cin_pad, int accumulate, float* dw, void* workspace, long long workspace_bytes, void* stream);
/* Host only: which kernel tt_conv2d_wgrad (x3 = 0) / tt_conv2d_wgrad_x3 (x3 = 1) would run these arguments on.  Runs the
 * validation and the dispatch of a launch and writes into `label` (label_bytes bytes, NUL-terminated)
 *   "<kernel with its template arguments, as rocprofv3 prints it> grid <x> x <y> lds <dynamic bytes> reduce <slices>"
 * followed, for a regrouped 1 x 1 layer, by " as N=.. OH=.. OW=.. H=.. W=.." (the geometry the kernel is launched with).
 * Dereferences no pointer (null-ness and alignment are all it looks at) and touches no device; returns the non-zero code,
 * with the error text, that the launch would return before launching. */
int tt_conv2d_wgrad_plan(const float* x, int N, int H, int W, int Cin, int x_cstride, int x_coff, const float* dy, int OH,
                         int OW, int Cout, int dy_cstride, int dy_coff, int KH, int KW, int stride, int pad, int dil,
                         int cin_pad, int accumulate, float* dw, void* workspace, long long workspace_bytes, int x3,
                         char* label, int label_bytes);
/* Backward of tt_conv2d_fwd's fused epilogue  y = act(scale[c]*conv + shift[c] + res1 + res2)  from dy and the saved
 * output y (all [M][*] channel-last f32 with channel stride / offset):  g = dy * act'(.)  (TT_ACT_NONE / RELU / SIGMOID);
 * dconv = g * scale[c] (feeds tt_conv2d_wgrad and the dgrad convolution); dres / dres2 (optional): g added to
 * (dres_accumulate) or written over the gradient windows of the two residual inputs -- overwrite is for a layer whose
 * output was written in place over its residual; dshift[c] (+)= sum_m g, dscale[c] (+)= sum_m g * conv (skipped when
 * scale is NULL; needs res1 / res2 to still hold their forward values).  Folded BatchNorm: dgamma = (dscale -
 * mean*dshift)/sigma, dbeta = dshift.  Deterministic. */
long long tt_conv_epilogue_bwd_workspace_bytes(int C);
int tt_conv_epilogue_bwd(const float* dy, int dy_cstride, int dy_coff, const float* y, int y_cstride, int y_coff,
                         const float* res1, int res1_cstride, int res1_coff, const float* res2, int res2_cstride,
                         int res2_coff, const float* scale, const float* shift, long long M, int C, int act, float* dconv,
                         int dconv_cstride, int dconv_coff, float* dres, int dres_cstride, int dres_coff, float* dres2,
                         int dres2_cstride, int dres2_coff, int dres_accumulate, float* dscale, float* dshift,
                         int accumulate, const int* m_dev_or_null, const float* pre_or_null, const float* conv_raw_or_null,
                         void* workspace, long long workspace_bytes, void* stream);
/* (pre_or_null: dense [M][C] pre-activation scale*conv + shift + res1 + res2, recomputed by running the layer once more
 *  without its activation -- required for GELU / softplus, whose derivative cannot be read off the output.
 *  conv_raw_or_null: dense [M][C] raw convolution output, recomputed likewise without scale / shift: dscale = sum g * conv
 *  is then exact; without it conv is reconstructed as (pre - shift - res) / scale, which loses everything when a BatchNorm
 *  gamma is (near) zero -- zero_init_residual, pruned channels -- or a sigmoid saturates; a zero scale contributes 0) */
/* Sparse (rulebook) convolution backward.  Weight gradient dw[co][0][t][ci] (+)= sum_m dy[m][co] * x[nbr[m][t]][ci] over the
 * live rows m < *m_dev (f32 MFMA, deterministic).  The input gradient is the forward gathered GEMM itself on a transposed
 * rulebook: for a submanifold layer the rulebook is its own transpose under tap reversal; for a strided layer
 * tt_sp_inverse_rulebook builds inv[j][t] = m  <=>  nbr[m][t] = j  (inv pre-filled with -1).  tt_sp_from_dense is the
 * backward of tt_sp_to_dense (gathers the dense gradient back to the rows, accumulating). */
long long tt_gather_conv_wgrad_workspace_bytes(long long M, int Cout, int Cin, int cin_pad, int taps);
int tt_gather_conv_wgrad(const float* x, int x_cstride, int Cin, const int* nbr, const int* m_dev, long long M, int taps,
                         const float* dy, int dy_cstride, int Cout, int cin_pad, int accumulate, float* dw, void* workspace,
                         long long workspace_bytes, void* stream);
/* Host only: tt_conv2d_wgrad_plan for the gathered layer (x3 is accepted and changes nothing: one arithmetic, exact f32). */
int tt_gather_conv_wgrad_plan(const float* x, int x_cstride, int Cin, const int* nbr, const int* m_dev, long long M, int taps,
                              const float* dy, int dy_cstride, int Cout, int cin_pad, int accumulate, float* dw,
                              void* workspace, long long workspace_bytes, int x3, char* label, int label_bytes);
int tt_sp_inverse_rulebook(const int* nbr, const int* m_dev, long long M, int taps, int* inv_prefilled_minus1, void* stream);
int tt_sp_from_dense(const float* gdense, const int* coords, const int* num_rows, long long max_rows, int C, int D, int H,
                     int W, float* grows, void* stream);
/* backward of tt_maxpool3x3s2 (F.max_pool2d(x,3,2,1)): dx[n][ih][iw][c] += sum of dy over the <= 4 windows whose FIRST
 * maximum (scan order kh, kw, as torch) is this pixel; gather form, no atomics */
int tt_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* backward of tt_upsample_nearest_add w.r.t. src: dsrc[n][sy][sx][c] += sum of ddst over the dst pixels that read (sy, sx) */
int tt_upsample_nearest_add_bwd(const float* ddst, float* dsrc, int N, int H, int W, int C, int h, int w, void* stream);
/* backward of tt_bilinear_up2 (x2, align_corners=True): dx [N][H][W][C] += weights^T dy [N][2H][2W][C] */
int tt_bilinear_up2_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* backward of tt_channel_gate (sigmoid gate): dx += g * s, dgate[n][c] += s(1-s) sum g*x, with g = dy, or -- when the
 * forward was out = relu(x*s + res), pass the saved out -- g = dy * [out > 0] and dres += g (optional) */
int tt_channel_gate_bwd(const float* x, const float* gate, const float* dy, float* dx, float* dgate, int N, int HW, int C,
                        const float* out_relu_or_null, float* dres_or_null, void* stream);
/* backward of tt_spatial_pool mode 1 (0.5 mean + 0.5 amax, ties share the amax gradient evenly); x dense [N][HW][C] */
int tt_spatial_meanmax_bwd(const float* x, const float* dpool, float* dx, int N, int HW, int C, void* stream);
/* backward of tt_spatial_pool mode 0 (mean): dx[n][p][coff + c] += dpool[n][c] / HW */
int tt_spatial_mean_bwd(const float* dpool, float* dx, int N, int HW, int C, int cstride, int coff, void* stream);
/* backward of tt_ew (same ops and row-strided channel windows): gv = dout * act'(saved out); da / db / dg (each optional)
 * are accumulated.  Activations: none, ReLU, sigmoid, softplus (from the saved output). */
int tt_ew_bwd(int op, int act, long long R, int C, const float* a, int a_stride, int a_coff, const float* b, int b_stride,
              int b_coff, const float* g, int g_stride, int g_coff, const float* out, int o_stride, int o_coff,
              const float* dout, int d_stride, int d_coff, float* da, int da_stride, int da_coff, float* db, int db_stride,
              int db_coff, float* dg, int dg_stride, int dg_coff, void* stream);
/* Backward of the look module's kernels (f32; the scatters add in a fixed order without atomics: bit-reproducible).  The waypoint / control inputs of a refinement layer
 * are detached in the reference (thinktwice_decoder.py:429-430), so there is no gradient for them or the reference points.
 * tt_look_gather_query_bwd: dout = gradient of the query rows; adds into the embeddings, the per-sample vectors and the four
 * FPN-side maps.  tt_msda_sample_bwd: adds into the value tensor's channel window, the offsets [R][512] and the attention
 * logits [R][256] (softmax included).  tt_sca_reduce_bwd: dx[bc][k] += dout[bc] / B for the slots the forward summed. */
int tt_look_gather_query_bwd(int B, const int* query_of_slot, const float* ref_packed, const float* dout, int row_stride,
                             float* dtemporal, float* dstatic, float* dmeas, float* dflat, float* const* dlevel_maps,
                             const int* level_hw, void* stream);
int tt_msda_sample_bwd(int B, const float* value, int value_cstride, int value_coff, const float* offsets,
                       const float* logits, const float* ref_packed, const int* level_hw, const float* dout, float* dvalue,
                       float* doffsets, float* dlogits, void* stream);
int tt_sca_reduce_bwd(int B, const float* dout, const int* max_len, float* dx, void* stream);
/* backward of tt_layernorm_rows: dx += , dgamma += , dbeta +=  (deterministic; workspace tt_layernorm_rows_bwd_workspace_bytes) */
long long tt_layernorm_rows_bwd_workspace_bytes(long long R, int D);
int tt_layernorm_rows_bwd(const float* x, const float* gamma, const float* dout, float* dx, float* dgamma, float* dbeta,
                          long long R, int D, int x_stride, int dout_stride, int dx_stride, float eps, void* workspace,
                          long long workspace_bytes, void* stream);
/* backward of one piece of tt_concat_rows: dsrc[(r / div) % mod or r / div][c] += dout[r][coff + c] summed over r */
int tt_concat_piece_bwd(const float* dout, int out_stride, int coff, long long R, int C, int div, int mod, float* dsrc,
                        int src_stride, int src_rows, void* stream);
/* backward of tt_broadcast_rows: dv[n][c] += sum_p dout[n][p][coff + c] */
int tt_broadcast_rows_bwd(const float* dout, float* dv, int N, int HW, int C, int cstride, int coff, int v_stride,
                          void* stream);
/* backward of tt_lift_splat_fwd (f32, rot_flip = 0): grad_out is the [B][Y][X][out_cstride] BEV gradient (channel window at
 * out_coff); grad_context [B*ncam][fH][fW][C] and grad_depth_logits [B*ncam][fH][fW][D] are accumulated (softmax included) */
int tt_lift_splat_bwd(int batch_size, int num_cams, int D, int fH, int fW, int C, int num_voxel_x, int num_voxel_y,
                      int num_voxel_z, const float* depth_logits, const float* context, const int32_t* geom_xyz,
                      const float* grad_out, int out_cstride, int out_coff, float* grad_depth_logits, float* grad_context,
                      void* stream);
/* backward of tt_deform_im2col3x3: gx += (no atomics: each channel's addends in (pixel, tap) order, bit-reproducible), goffsets[pix][2 tap (+1)] += the sampling-position gradients */
int tt_deform_im2col3x3_bwd(const float* x, const float* offsets, const float* gcols, float* gx, float* goffsets, int N,
                            int H, int W, int C, int off_cstride, int pad, void* stream);

/* SURVEY 8f-1, LiDAR side: merge of the two 180-degree half sweeps of the closed-loop tick
 * (leaderboard/team_code/thinktwice_agent.py:340-352).  prev / now: (n, 4) f32 (x, y, z, intensity) device rows;
 * rel_transform_3x4: HOST pointer to the first three rows of inv(T_now) @ T_prev (row-major); out: (n_prev + n_now, 4)
 * = [transformed prev | now] with z += z_shift (2.5). */
int tt_lidar_merge_half_sweeps(const float* prev_xyzi, int n_prev, const float* now_xyzi, int n_now,
                               const float* rel_transform_3x4, float z_shift, float* out_xyzi, void* stream);

/* ------------------------------------------------------------------------
 * The multi-sweep cloud of a TRAINING batch: union2one's "dense-fusion" (open_loop_training/code/datasets/carla_dataset.py:
 * 314-328) for every sample of a batch, and the zero rows mmcv's collate pads the ragged clouds with, in one launch.
 *
 * points_xyzi: device f32 rows (x, y, z, intensity), `num_rows` of them, base 16-byte aligned.  `sweeps` is a HOST pointer to
 * B * T tt_union_sweep, entry b * T + t for sweep t of sample b (t = T - 1 is the key sweep, t = 0 the oldest): rows
 * first_row .. first_row + count - 1 of points_xyzi, in any order, with gaps, count = 0 allowed.  The entry checks every
 * segment and copies the table into the kernel's arguments (by value, like tt_ida_set: no device buffer, no copy, no
 * synchronisation, no workspace), which bounds a call to TT_UNION_MAX_SWEEPS = B * T sweeps.
 *
 * out f32 [B, Np, 5]; for sample b, in this order:
 *   key sweep     the rows of sweep T - 1 copied bit for bit, column 4 = 0.0; its matrix is NOT read (:315-318)
 *   older sweeps  for t = T - 2 .. 0 the rows of sweep t, columns 0..3 = M[b, t] . (x, y, z, i) -- all four rows of the
 *                 matrix, the intensity in the place of the homogeneous coordinate (:323) --, column 4 = (float)(t - (T - 1))
 *   padding       every remaining row up to Np: five +0.0 (the caller does not clear `out`)
 * A transformed component j is, in f32:  fmaf(m[4j+3], i, fmaf(m[4j+2], z, fmaf(m[4j+1], y, m[4j] * x)))  -- one rounded
 * product, then three fused multiply-adds in column order -- so the result is defined and the same from run to run.
 *
 * Returns an error, before any launch, for: a null `sweeps` or `out`, a null `points_xyzi` with a non-empty segment or one
 * that is not 16-byte aligned; B < 1, T < 2, Np < 0; B * T > TT_UNION_MAX_SWEEPS; a negative first_row or count, a segment
 * that ends after num_rows; a sample whose counts sum to more than Np; B * Np above 2^31 - 1024 (the kernel indexes
 * output rows with an int).
 * ---------------------------------------------------------------------- */
#define TT_UNION_MAX_SWEEPS 32
typedef struct tt_union_sweep {
    long long first_row;        /* first row of the segment in points_xyzi */
    int count;                  /* rows of the segment */
    int reserved;               /* (keeps the matrix at offset 16; not read) */
    float m[16];                /* row-major 4x4 curr2key of the sweep; not read for the key sweep */
} tt_union_sweep;               /* 80 bytes */
int tt_lidar_union_sweeps(const float* points_xyzi, long long num_rows, const tt_union_sweep* sweeps, int B, int T, int Np,
                          float* out, void* stream);

/* ------------------------------------------------------------------------
 * train-mode BatchNorm (batch statistics) over channel-last rows -- what every nn.BatchNorm2d / BatchNorm1d
 * (torch.nn.SyncBatchNorm under configs/thinktwice.py:39 SyncBN=True, apis/mmdet_train.py:86-87) computes under
 * model.train() (norm_eval=False, configs/thinktwice.py:146).  The convolution in front writes its raw output z (bias in);
 * `groups` equal row groups are normalised with their own statistics (the camera trunk's T sweeps run as one batch here,
 * one pass per sweep in the reference, lss.py:690-717); m_dev != NULL: sparse rows, live count on the device, groups == 1.
 *   stats  : double [groups][2C + 2] = per-channel sum | sum of squares | row count | 0 -- the block a SyncBN all-reduce
 *            (SUM) runs over, between tt_bn_stats and tt_bn_finalize
 *   scale (= gamma * invstd) / shift (= beta) / mean / invstd : float [groups][C]; running_mean / running_var (nullable) are updated like torch does
 *            (momentum, unbiased variance), group 0 (the key sweep) first, like lss.py:689-714
 *   tt_bn_apply      out[m][out_coff + c] = act((z - mean) * scale + shift + res1 + res2), act in {TT_ACT_NONE, TT_ACT_RELU}
 *            (centred like torch: folding the mean into the shift loses ulp(mean * scale) where the variance is ~0)
 *   tt_bn_bwd_reduce dy := dy * act'(y) in place, dres += it, sums = double [groups][2C] = sum g | sum g * xhat (LOCAL;
 *            dgamma / dbeta are these; under SyncBN they are all-reduced before tt_bn_bwd_apply)
 *   tt_bn_bwd_apply  dz = scale * (g - sum_g / n - xhat * sum_gxhat / n), n = stats[g][2C]
 * ---------------------------------------------------------------------- */
long long tt_bn_workspace_bytes(int C, int groups);
int tt_bn_stats(const float* z, long long M, int C, int z_cstride, int z_coff, const int* m_dev, int groups, double* stats,
                void* workspace, long long workspace_bytes, void* stream);
int tt_bn_finalize(const double* stats, int C, int groups, const float* gamma, const float* beta, float eps, float momentum,
                   float* running_mean, float* running_var, float* scale, float* shift, float* mean, float* invstd,
                   void* stream);
int tt_bn_apply(const float* z, long long M, int C, int z_cstride, int z_coff, const int* m_dev, int groups,
                const float* scale, const float* shift, const float* mean, const float* res1, int r1_cstride, int r1_coff, const float* res2,
                int r2_cstride, int r2_coff, int act, float* out, int out_cstride, int out_coff, void* stream);
int tt_bn_bwd_reduce(float* dy, int dy_cstride, int dy_coff, const float* y, int y_cstride, int y_coff, const float* z,
                     int z_cstride, int z_coff, long long M, int C, const int* m_dev, int groups, const float* mean,
                     const float* invstd, int act, float* dres1, int d1_cstride, int d1_coff, float* dres2, int d2_cstride,
                     int d2_coff, double* sums, void* workspace, long long workspace_bytes, void* stream);
int tt_bn_bwd_apply(const float* g, int g_cstride, int g_coff, const float* z, int z_cstride, int z_coff, long long M, int C,
                    const int* m_dev, int groups, const double* sums, const double* stats, const float* scale,
                    const float* mean, const float* invstd, float* dz, int dz_cstride, int dz_coff, void* stream);
/* nn.Dropout(p) of the DepthNet ASPP (lss.py:91,110) in train mode: keep-mask from a counter-based generator (seed, element
 * index -> splitmix64), out = x * mask / (1 - p); `mask` (uint8 [n], nullable) receives the keep bits for the backward, or --
 * mask_in != NULL -- supplies them (parity tests replay the reference's torch mask). */
int tt_dropout_fwd(const float* x, float* out, long long n, float p, unsigned long long seed, const uint8_t* mask_in,
                   uint8_t* mask_out, void* stream);
int tt_dropout_bwd(const float* dout, const uint8_t* mask, float* dx, long long n, float p, void* stream);

/* ------------------------------------------------------------------------
 * action post-processing of a closed-loop tick, on the device (one thread) or on the host.
 * Replaces, in ONE call:
 *   EncoderDecoder.process_action / _get_action_beta  (code/encoder_decoder_framework.py:268-304): Beta mode of the last
 *       refinement stage's control branch -> (steer, throttle, brake)_ctrl;
 *   EncoderDecoder.control_pid + PIDController.step   (encoder_decoder_framework.py:309-390, code/utils.py:7-29): waypoint
 *       PID with its two n-entry error windows -> (steer, throttle, brake)_traj;
 *   the agent's arbitration + stuck detector          (leaderboard/team_code/thinktwice_agent.py:463-509)
 *       -> the final (steer, throttle, brake).
 * The reference copies mu / sigma / waypoints to the host and does this in numpy; here the model outputs are read where
 * they are and a tick needs exactly one small device->host copy (`out`).
 *   cfg    : the reference's `cfg` scalars (configs/thinktwice.py:44-57) + stuck_threshold (thinktwice_agent.py: 800).
 *   state  : caller-owned; zero-initialised == the reference's fresh deques ([0]*n) and stuck_detector = 0.
 *   mu_last / sigma_last : 2 floats each = pred['mu_branches'][0, -1, :], pred['sigma_branches'][0, -1, :]
 *   wp_last: 8 floats = pred['pred_wp'][0, -1, :, :] (4 waypoints x (x, y));  target_xy: 2 floats.
 *   stuck_desired_speed <= 0: unused (the reference's default -1).
 *   out    : TT_ACTION_OUT doubles, see the index names below.
 * tt_action_post: mu/sigma/wp/state/out are DEVICE pointers, target/speed by value; asynchronous on `stream`.
 * tt_action_post_host: every pointer is a HOST pointer; no GPU involved (same arithmetic, same source).
 * ---------------------------------------------------------------------- */
#define TT_PID_WINDOW_MAX 64
typedef struct tt_action_cfg {
    double turn_KP, turn_KI, turn_KD, speed_KP, speed_KI, speed_KD;
    double brake_speed, brake_ratio, clip_delta, aim_dist, angle_thresh, dist_thresh;
    int turn_n, speed_n, stuck_threshold, reserved;
} tt_action_cfg;
typedef struct tt_action_state {
    double turn_window[TT_PID_WINDOW_MAX], speed_window[TT_PID_WINDOW_MAX];
    int turn_head, speed_head;      /* ring position of the OLDEST entry (= where the next error is written) */
    int stuck_detector, reserved;
} tt_action_state;
enum {
    TT_ACT_STEER = 0, TT_ACT_THROTTLE, TT_ACT_BRAKE,                 /* the final control of the tick            */
    TT_ACT_STEER_CTRL, TT_ACT_THROTTLE_CTRL, TT_ACT_BRAKE_CTRL,      /* process_action                           */
    TT_ACT_STEER_TRAJ, TT_ACT_THROTTLE_TRAJ, TT_ACT_BRAKE_TRAJ,      /* control_pid (brake: 0 / 1)               */
    TT_ACT_DESIRED_SPEED, TT_ACT_ANGLE, TT_ACT_ANGLE_LAST, TT_ACT_ANGLE_TARGET, TT_ACT_ANGLE_FINAL, TT_ACT_DELTA,
    TT_ACT_AIM_X, TT_ACT_AIM_Y,                                      /* control_pid metadata                     */
    TT_ACT_IS_TURN, TT_ACT_IS_STUCK, TT_ACT_STUCK_DETECTOR,          /* arbitration                              */
    TT_ACTION_OUT = 24
};
int tt_action_post(const float* mu_last, const float* sigma_last, const float* wp_last, float speed, float target_x,
                   float target_y, float stuck_desired_speed, const tt_action_cfg* cfg_host, tt_action_state* state,
                   double* out, void* stream);
int tt_action_post_host(const float* mu_last, const float* sigma_last, const float* wp_last, float speed, float target_x,
                        float target_y, float stuck_desired_speed, const tt_action_cfg* cfg, tt_action_state* state,
                        double* out);
/* the three stages one by one on the host, for callers that keep the reference's call structure (process_action, then
 * control_pid, then the agent's own arbitration): each fills its slots of `out` (the rest is zeroed) */
int tt_action_ctrl_host(const float* mu_last, const float* sigma_last, double* out);
int tt_action_pid_host(const float* wp_last, float speed, float target_x, float target_y, float stuck_desired_speed,
                       const tt_action_cfg* cfg, tt_action_state* state, double* out);
/* the arbitration stage alone (thinktwice_agent.py:463-509), for a host that already holds the two heads' controls:
 * fills TT_ACT_STEER / THROTTLE / BRAKE / IS_TURN / IS_STUCK / STUCK_DETECTOR of `out`, updates state->stuck_detector */
int tt_action_arbitrate_host(double steer_ctrl, double throttle_ctrl, double brake_ctrl, double throttle_traj,
                             double brake_traj, float speed, const tt_action_cfg* cfg, tt_action_state* state, double* out);

/* ------------------------------------------------------------------------
 * launch plans -- the forward sequenced from C (csrc/plan.cpp).
 * The reference sequences the forward in Python (encoder_decoder_framework.py:194-250: extract_sensor_feat ->
 * get_fusion_feat -> ThinkTwiceDecoder.forward, thinktwice_decoder.py:419-489).  A plan is that sequence as data: the ordered
 * C-ABI calls of one forward, every pointer as (buffer id, byte offset) -- buffer 0 = packed weights, 1 = activation arena,
 * 2.. = inputs -- the stream slot of each call and the cross-stream dependencies.  thinktwice_amd/plan.py compiles a plan by
 * recording one forward of the Python mirror; this runtime binds a host's buffers and issues the calls on its streams.  Plans
 * (and the weights blob) are files: a non-Python host runs the path with tt_plan_load + tt_plan_bind + tt_encoder_fwd /
 * tt_decoder_fwd (tools/plan_host.cpp).  Argument kinds of tt_plan_add_call: 0 = integer (ivals), 1 = float / double (fvals),
 * 2 = device pointer (buffers[i], ivals[i] = byte offset), 3 = host blob (ivals[i] = offset returned by tt_plan_add_blob;
 * device pointers stored inside a blob are declared with tt_plan_add_reloc), 4 = NULL.
 * ---------------------------------------------------------------------- */
/* buffer plumbing as C-ABI entries, so that a plan holds NO torch kernel: zeros / constant fills (32-bit pattern) and
 * contiguous device-to-device copies */
int tt_fill_u32(void* dst, long long n_words, unsigned pattern, void* stream);
int tt_copy_bytes(void* dst, const void* src, long long nbytes, void* stream);
typedef struct tt_plan tt_plan;
tt_plan* tt_plan_create(void);
void tt_plan_destroy(tt_plan* plan);
int tt_plan_set_buffer(tt_plan* plan, int id, long long bytes, const char* name);
long long tt_plan_add_blob(tt_plan* plan, const void* bytes, long long n);
int tt_plan_add_reloc(tt_plan* plan, long long blob_offset, int buffer, long long offset);
int tt_plan_add_call(tt_plan* plan, const char* entry, int nargs, const int* kinds, const int* buffers, const long long* ivals,
                     const double* fvals, int stream_slot);
int tt_plan_add_sync(tt_plan* plan, int waiter_stream_slot, int signal_stream_slot);
/* Builder only.  Declare one allocation of the activation arena (address order, no overlap), then let the plan re-place the
 * allocations by liveness: tt_plan_compact_arena rewrites every pointer into buffer `arena_buffer` (call arguments, pointers
 * inside argument blobs, outputs) and returns the arena's new size in bytes (< 0 on error, plan unchanged).  Memory is handed
 * on only between allocations whose every use is on ONE stream (stream order makes the reuse safe); outputs keep their own.
 * (replaces the caching allocator torch gives the reference's eager forward, encoder_decoder_framework.py:194-235) */
int tt_plan_add_arena_alloc(tt_plan* plan, long long offset, long long nbytes);
long long tt_plan_compact_arena(tt_plan* plan, int arena_buffer, long long align);
/* outputs: where a host finds a result tensor -- byte offset of element 0 inside `buffer`, shape and ELEMENT strides (f32) */
int tt_plan_add_output(tt_plan* plan, const char* name, int buffer, long long offset, int ndim, const long long* shape,
                       const long long* stride);
int tt_plan_num_ops(const tt_plan* plan);
int tt_plan_num_calls(const tt_plan* plan);
int tt_plan_num_streams(const tt_plan* plan);
int tt_plan_num_buffers(const tt_plan* plan);
long long tt_plan_buffer_bytes(const tt_plan* plan, int id);
const char* tt_plan_buffer_name(const tt_plan* plan, int id);
int tt_plan_num_outputs(const tt_plan* plan);
int tt_plan_output(const tt_plan* plan, int i, const char** name, int* buffer, long long* offset, int* ndim, long long* shape8,
                   long long* stride8);
int tt_plan_save(const tt_plan* plan, const char* path);
tt_plan* tt_plan_load(const char* path);
/* bases[id]: device (or, for host-read arguments, host) address of buffer id, tt_plan_buffer_bytes(id) bytes each */
int tt_plan_bind(tt_plan* plan, void* const* bases, int nbases);
/* issue the whole plan / one half on the caller's streams (hipStream_t as void*), asynchronously */
int tt_plan_run(tt_plan* plan, void* const* streams, int nstreams);
int tt_plan_run_range(tt_plan* plan, void* const* streams, int nstreams, int first_op, int num_ops);
/* the encoder half (camera + LiDAR encoders, BEV fusion + flatten network: encoder_decoder_framework.py:194-235) and the
 * decoder half (ThinkTwiceDecoder.forward, thinktwice_decoder.py:419-489) of a bound forward plan */
int tt_encoder_fwd(tt_plan* plan, void* const* streams, int nstreams);
int tt_decoder_fwd(tt_plan* plan, void* const* streams, int nstreams);

#ifdef __cplusplus
}
#endif
#endif /* THINKTWICE_HIP_H */
