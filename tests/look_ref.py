"""Float64 references and input generators of the look-module parity tests (test_look_ref.py, test_look_ops.py,
test_look_bwd.py); the tolerance rules, the guarded buffers and the report are those of glue_ref.py.

Everything here runs on the CPU.  The operations of csrc/look_module.hip are restated in plain torch from their descriptions
(project the 120 look points into the four cameras and left-pack the in-image ones; assemble the 1543-wide query rows; the
multi-scale deformable attention core; the batch-coupled slot reduction), differentiable where csrc/look_bwd.hip has a
backward; test_look_ref.py holds them to oracle/model_ref.py (project_queries, msda_core, look_module) in float64.

Layouts (R = B * 4 * 120 rows, row = (b * 4 + cam) * 120 + slot):
  value    [B*4][S][256]      the level maps one after the other, S = sum H_l W_l, channel = head * 32 + c
  offsets  [R][512]           (head, level, point, xy) in PIXELS of the level
  logits   [R][256]           (head, level * 8 + point); softmax over the 32 of a head
  query    [R][1543]          [ctrl4 | xyz3 | emb128 | meas128 | flat256 | 1024 samples, channel-major level-minor]"""
import functools

import torch
import torch.nn.functional as F

from glue_ref import check, check_equal, Win, prefill, PREFILL_ULP, sum_bound, f32_limit, vjp, fit_scale, SENT  # noqa: F401
from glue_ref import U32, layernorm_bound  # noqa: F401

Q, CAMS = 120, 4
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))        # the in-front-of-the-camera threshold as the device holds it
STATIC_XY = ((5.0, 0.0), (0.0, -5.0), (0.0, 5.0), (-5.0, 0.0))


# ----------------------------------------------------------------------------- projection and packing
def look_points(wp):
    """wp (B,4,2) -> (B,120,3): query q = point * 15 + height; points 0..3 the waypoints, 4..7 the static ones; z = -4 .. 10."""
    B = wp.shape[0]
    xy = torch.cat([wp.double(), torch.tensor(STATIC_XY, dtype=torch.float64).expand(B, 4, 2)], 1)
    z = torch.arange(15, dtype=torch.float64) - 4.0
    return torch.cat([xy.unsqueeze(2).expand(B, 8, 15, 2), z.view(1, 1, 15, 1).expand(B, 8, 15, 1)], -1).reshape(B, Q, 3)


def project_ref(wp, lidar2img, ida, img_hw):
    """Float64 projection of the look points: rx, ry, iz (B,4,120) and their running error bounds brx, bry, biz: the same
    expression on absolute values times 8 * 2^-24 (a quotient also carries the bound of its denominator)."""
    B = wp.shape[0]
    p = torch.cat([look_points(wp), torch.ones(B, Q, 1, dtype=torch.float64)], -1).view(B, 1, Q, 4)
    Lm, A = lidar2img.double().view(B, CAMS, 1, 4, 4), ida.double().view(B, CAMS, 1, 4, 4)
    cam = (Lm * p.unsqueeze(-2)).sum(-1)                                                   # (B,4,120,4)
    cam_a = (Lm.abs() * p.abs().unsqueeze(-2)).sum(-1)
    cz = cam[..., 2]
    zz = cz.clamp(min=EPS32)
    zz_a = torch.where(cz > EPS32, cam_a[..., 2], torch.zeros_like(cz))                    # the clamp value itself is exact
    u = cam[..., :2] / zz.unsqueeze(-1)
    u_a = cam_a[..., :2] / zz.unsqueeze(-1) + u.abs() * (zz_a / zz).unsqueeze(-1)
    v = torch.cat([u, cam[..., 2:]], -1)
    v_a = torch.cat([u_a, cam_a[..., 2:]], -1)
    img = (A * v.unsqueeze(-2)).sum(-1)
    img_a = (A.abs() * v_a.unsqueeze(-2)).sum(-1)
    k = 8.0 * U32
    return (img[..., 0] / img_hw[1], img[..., 1] / img_hw[0], img[..., 2],
            k * img_a[..., 0] / img_hw[1], k * img_a[..., 1] / img_hw[0], k * img_a[..., 2])


def ambiguous_points(wp, lidar2img, ida, img_hw):
    """Points whose in-image decision the f32 rounding could flip: rx or ry within its bound of 0 or 1, iz within its bound of 1e-5."""
    rx, ry, iz, brx, bry, biz = project_ref(wp, lidar2img, ida, img_hw)
    return ((rx.abs() <= brx) | ((rx - 1).abs() <= brx) | (ry.abs() <= bry) | ((ry - 1).abs() <= bry) | ((iz - EPS32).abs() <= biz))


def project_pack_ref(wp, lidar2img, ida, img_hw):
    """-> ref_packed (B,4,120,2) float64, query_of_slot (B,4,120) int32, count (B,4) int32, max_len, bound (B,4,120,2): the
    in-image points (all five comparisons strict) of every (sample, camera) moved to the front in query order; padded slots
    are -1 and (0, 0).  `bound` is the error bound of ref_packed, packed the same way."""
    rx, ry, iz, brx, bry, _ = project_ref(wp, lidar2img, ida, img_hw)
    ok = (iz > EPS32) & (ry > 0) & (ry < 1) & (rx < 1) & (rx > 0)
    B = wp.shape[0]
    packed = torch.zeros(B, CAMS, Q, 2, dtype=torch.float64)
    bound = torch.zeros(B, CAMS, Q, 2, dtype=torch.float64)
    qos = torch.full((B, CAMS, Q), -1, dtype=torch.int32)
    count = ok.sum(-1).to(torch.int32)
    for b in range(B):
        for c in range(CAMS):
            qs = torch.nonzero(ok[b, c]).reshape(-1)
            n = qs.numel()
            qos[b, c, :n] = qs.to(torch.int32)
            packed[b, c, :n, 0], packed[b, c, :n, 1] = rx[b, c, qs], ry[b, c, qs]
            bound[b, c, :n, 0], bound[b, c, :n, 1] = brx[b, c, qs], bry[b, c, qs]
    return packed, qos, count, int(count.max()), bound


def dyadic_projection_case(B):
    """Matrices with small-integer / power-of-two entries, the depth cz a power of two wherever it is positive, waypoints on a
    1/4 grid, a 128 x 256 image: the f32 evaluation of every in-front point is exact.  Per sample:
      camera 0  rx = (4 X + 128) / 256, ry = (8 Z + 40) / 128       : all 120 inside (64 in the first ballot, 56 in the second)
      camera 1  as camera 0 but iz = 1e-5f * cz = 1e-5f exactly     : none inside (the comparison is strict)
      camera 2  cz = -Z - 2 (2, 1, 0, then behind the camera)       : heights 0 and 1 of every point: 10 + 6 across the ballots
      camera 3  rx = (8 X + 128) / 256, ry = (16 Z + 64) / 128      : waypoints at X = -16 / +16 give rx == 0 / rx == 1, heights
                                                                      -4 / +4 give ry == 0 / ry == 1, heights above 4 are outside"""
    wp = torch.tensor([[-16.0, 1.25], [16.0, -2.5], [3.25, 0.75], [-7.5, -5.75]]).repeat(B, 1, 1)
    wp[:, 2, 0] += torch.arange(B).float()
    wp[:, 3, 1] += 0.25 * torch.arange(B).float()

    def mat(rows):
        return torch.tensor(rows, dtype=torch.float32)
    eye = torch.eye(4)
    l2i = torch.stack([mat([[4, 0, 0, 128], [0, 0, 8, 40], [0, 0, 0, 1], [0, 0, 0, 1]]),
                       mat([[4, 0, 0, 128], [0, 0, 8, 40], [0, 0, 0, 1], [0, 0, 0, 1]]),
                       mat([[8, 0, 0, 128], [0, 8, 0, 64], [0, 0, -1, -2], [0, 0, 0, 1]]),
                       mat([[8, 0, 0, 128], [0, 0, 16, 64], [0, 0, 0, 1], [0, 0, 0, 1]])])
    ida = torch.stack([eye, eye.clone(), eye, eye])
    ida[1, 2, 2] = EPS32
    return wp, l2i.repeat(B, 1, 1, 1).contiguous(), ida.repeat(B, 1, 1, 1).contiguous(), (128, 256)


PROJ_SEEDS = (0, 1, 2)


def random_projection_case(B, seed):
    """The evaluation rig's intrinsics and extrinsics with per-(sample, camera) jitter and waypoints a few metres ahead.  The
    seeds in PROJ_SEEDS leave no ambiguous point (test_look_ref.py asserts it)."""
    from oracle import lss_geometry as og
    from thinktwice_amd import synth
    hw = (128, 256)
    _, _, _, l2i, ida = og.assemble_camera_mats(synth.make_img_metas(B, final_dim=hw, jitter_seed=100 + seed))
    g = torch.Generator().manual_seed(seed)
    wp = torch.randn(B, 4, 2, generator=g) * torch.tensor([6.0, 3.0]) + torch.tensor([4.0, 0.0])
    return wp, l2i.float().contiguous(), ida.float().contiguous(), hw


# ----------------------------------------------------------------------------- bilinear sampling
def bilinear_corners(x, y, H, W):
    """Pixel coordinates (any shape) -> idx (..., 4) flat position y * W + x of the four corners (clamped), w (..., 4) their
    weights, valid (..., 4).  floor; corner order (y0,x0) (y0,x1) (y1,x0) (y1,x1); a corner outside the map is zero padding."""
    x0, y0 = torch.floor(x).detach(), torch.floor(y).detach()
    lx, ly = x - x0, y - y0
    cx = torch.stack([x0, x0 + 1, x0, x0 + 1], -1)
    cy = torch.stack([y0, y0, y0 + 1, y0 + 1], -1)
    w = torch.stack([(1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx], -1)
    valid = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
    idx = cy.clamp(0, H - 1).long() * W + cx.clamp(0, W - 1).long()
    return idx, w, valid


def bilinear_cl_ref(fmap, nx, ny):
    """fmap (N,H,W,C) channel-last, normalised coordinates nx, ny (N,K) -> (N,K,C): the explicit four-corner gather with
    align_corners=False (pixel x = nx * W - 0.5), zero padding and floor.  At an exactly integral pixel coordinate floor takes
    the coordinate itself, the weight of the right-hand corner is 0 and grows with the coordinate: the derivative with
    respect to the coordinate is the RIGHT-HAND one, (v[x0 + 1] - v[x0]).  This is F.grid_sample's convention."""
    N, H, W, C = fmap.shape
    idx, w, valid = bilinear_corners(nx * W - 0.5, ny * H - 0.5, H, W)                     # (N,K,4)
    vals = fmap.reshape(N, H * W, C)[torch.arange(N).view(N, 1, 1), idx]                   # (N,K,4,C)
    return ((w * valid).unsqueeze(-1) * vals).sum(2)


# ----------------------------------------------------------------------------- query rows
def gather_query_ref(qos, ref, wp, ctrl, temporal, static, meas, flat, maps, raw_ctrl=False):
    """-> (B*4*120, 1543): the query rows of every slot; zero rows where query_of_slot < 0.  maps: four (B*4,H,W,256)
    channel-last tensors; `ctrl` (B,4,4) is softplus'ed here when raw_ctrl.  Differentiable in temporal, static, meas, flat
    and the maps (the waypoints, the control values and the reference points are detached in the model)."""
    B = wp.shape[0]
    dt = flat.dtype
    q = qos.reshape(B, CAMS, Q).long()
    live = (q >= 0)
    qc = q.clamp(min=0)
    pt, zi = qc // 15, qc % 15
    bI = torch.arange(B).view(B, 1, 1).expand(B, CAMS, Q)
    c = F.softplus(ctrl.to(dt)) if raw_ctrl else ctrl.to(dt)
    c8 = torch.cat([c, torch.zeros(B, 4, 4, dtype=dt)], 1)[bI, pt]                         # (B,4,120,4)
    xy = torch.cat([wp.to(dt), torch.tensor(STATIC_XY, dtype=dt).expand(B, 4, 2)], 1)[bI, pt]
    z = (zi.to(dt) - 4.0).unsqueeze(-1)
    emb = torch.cat([temporal, static], 0)[pt]                                             # (B,4,120,128)
    r = ref.to(dt).reshape(B * CAMS, Q, 2)
    samp = torch.stack([bilinear_cl_ref(m, r[..., 0], r[..., 1]) for m in maps], -1)       # (BC,120,256,4)
    rows = torch.cat([c8, xy, z, emb, meas[bI], flat[bI], samp.reshape(B, CAMS, Q, 1024)], -1)
    return (rows * live.unsqueeze(-1).to(dt)).reshape(B * CAMS * Q, 1543)


def layer_norm(x, gamma, beta, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), gamma, beta, eps)


def look_query_ln_ref(gamma, beta, *a, eps=1e-5, **k):
    return layer_norm(gather_query_ref(*a, **k), gamma, beta, eps)


# ----------------------------------------------------------------------------- deformable attention core
def msda_pixels(offsets, ref, level_hw):
    """Pixel coordinates of every sample: x, y (R, 8 heads, 4 levels, 8 points); x = (rx + off_x / W) * W - 0.5."""
    R = offsets.shape[0]
    off = offsets.reshape(R, 8, 4, 8, 2)
    Wl = torch.tensor([w for _, w in level_hw], dtype=offsets.dtype).view(1, 1, 4, 1)
    Hl = torch.tensor([h for h, _ in level_hw], dtype=offsets.dtype).view(1, 1, 4, 1)
    x = (ref[:, 0].view(R, 1, 1, 1) + off[..., 0] / Wl) * Wl - 0.5
    y = (ref[:, 1].view(R, 1, 1, 1) + off[..., 1] / Hl) * Hl - 0.5
    return x, y


def msda_coord_err(offsets, ref, level_hw):
    """Bound of the f32 rounding of a sample's pixel coordinates, x and y together (R,8,4,8): x = (rx + off / W) * W - 0.5 takes
    four roundings, of off / W, of the sum, of the product and of the difference: <= 4 * 2^-24 (|rx| W + |off| + 1)."""
    R = offsets.shape[0]
    off = offsets.double().reshape(R, 8, 4, 8, 2).abs()
    Wl = torch.tensor([w for _, w in level_hw], dtype=torch.float64).view(1, 1, 4, 1)
    Hl = torch.tensor([h for h, _ in level_hw], dtype=torch.float64).view(1, 1, 4, 1)
    r = ref.double().abs()
    return 4 * U32 * ((r[:, 0].view(R, 1, 1, 1) * Wl + off[..., 0] + 1) + (r[:, 1].view(R, 1, 1, 1) * Hl + off[..., 1] + 1))


def msda_ref(value, offsets, logits, ref, level_hw, coff=0, corner_w=None):
    """value (B*4, S, >= coff + 256), offsets (R,512), logits (R,256), ref (R,2) -> (R,256):
    out[row, head*32 + c] = sum_{level, point} softmax(logits of the head) * bilinear(value level map, channel head*32 + c).
    `corner_w` (R,8,4,8) replaces the bilinear weight of every in-map corner (the error bounds of the backward tests)."""
    BC, S = value.shape[0], value.shape[1]
    R = offsets.shape[0]
    assert R == BC * Q and S == sum(h * w for h, w in level_hw)
    v = value[..., coff:coff + 256].reshape(BC, S, 8, 32)
    attw = logits.reshape(R, 8, 32).softmax(-1).reshape(BC, Q, 8, 4, 8)
    x, y = msda_pixels(offsets, ref, level_hw)
    x, y = x.reshape(BC, Q, 8, 4, 8), y.reshape(BC, Q, 8, 4, 8)
    bI, hI = torch.arange(BC).view(BC, 1, 1, 1, 1), torch.arange(8).view(1, 1, 8, 1, 1)
    out, start = 0, 0
    for lv, (H, W) in enumerate(level_hw):
        idx, w, valid = bilinear_corners(x[:, :, :, lv], y[:, :, :, lv], H, W)            # (BC,Q,8,8,4)
        vals = v[:, start:start + H * W][bI, idx, hI]                                      # (BC,Q,8,8,4,32)
        if corner_w is not None:
            w = corner_w.reshape(BC, Q, 8, 4, 8)[:, :, :, lv].unsqueeze(-1).expand_as(w)
        s = ((w * valid).unsqueeze(-1) * vals).sum(4)                                      # (BC,Q,8,8,32)
        out = out + (attw[:, :, :, lv].unsqueeze(-1) * s).sum(3)
        start += H * W
    return out.reshape(R, 256)


def msda_touch_count(offsets, ref, level_hw, BC):
    """How many (row, sample, corner) triples land on every position of the value tensor, per head: (BC, S, 8) float64."""
    S = sum(h * w for h, w in level_hw)
    x, y = msda_pixels(offsets.double(), ref.double(), level_hw)
    x, y = x.reshape(BC, Q, 8, 4, 8), y.reshape(BC, Q, 8, 4, 8)
    cnt = torch.zeros(BC * S * 8, dtype=torch.float64)
    start = 0
    for lv, (H, W) in enumerate(level_hw):
        idx, _, valid = bilinear_corners(x[:, :, :, lv], y[:, :, :, lv], H, W)
        flat = ((torch.arange(BC).view(BC, 1, 1, 1, 1) * S + start + idx) * 8 + torch.arange(8).view(1, 1, 8, 1, 1))
        cnt.index_add_(0, flat[valid], torch.ones(int(valid.sum()), dtype=torch.float64))
        start += H * W
    return cnt.reshape(BC, S, 8)


def project_value(maps, weight, bias, vshift):
    """value_proj of EVERY position: maps four (B*4,H,W,256), weight (out,in), bias (256), vshift (level, camera, 256)
    -> (B*4, S, 256); camera = map index % 4."""
    BC = maps[0].shape[0]
    cam = torch.arange(BC) % CAMS
    return torch.cat([(m.reshape(BC, -1, 256) @ weight.t() + bias + vshift[lv][cam].unsqueeze(1)) for lv, m in enumerate(maps)], 1)


def msda_proj_ref(maps, offsets, logits, ref, weight, bias, vshift):
    """The sample-first kernel's result in the reference's order: project every position, then sample."""
    level_hw = [(m.shape[1], m.shape[2]) for m in maps]
    return msda_ref(project_value(maps, weight, bias, vshift), offsets, logits, ref, level_hw)


# ----------------------------------------------------------------------------- slot reduction and the merge row
def sca_reduce_ref(x, max_len, B):
    """x (B*4*120, 256) -> (B, 1024): sum_{k = B}^{min(max_len, 120) - 1} x[bc, k, :] / B, (camera, channel) per sample."""
    hi = min(int(max_len), Q)
    xs = x.reshape(B * CAMS, Q, 256)[:, B:hi] if hi > B else x.reshape(B * CAMS, Q, 256)[:, :0]
    return (xs / B).sum(1).reshape(B, CAMS * 256)


def merge_in_cat(fflat, look, temporal, meas):
    """Row (b, t) of a refinement layer's mlp input before its LayerNorm: [future flat (b,t) 256 | look (b) 256 | zeros 256 |
    temporal (t) 128 | measurement (b) 128]."""
    B = look.shape[0]
    return torch.cat([fflat.reshape(B, 4, 256), look.unsqueeze(1).expand(B, 4, 256), torch.zeros(B, 4, 256, dtype=look.dtype),
                      temporal.unsqueeze(0).expand(B, 4, 128), meas.unsqueeze(1).expand(B, 4, 128)], -1).reshape(B * 4, 1024)


def merge_in_ref(fflat, look, temporal, meas, gamma, beta, eps=1e-5):
    return layer_norm(merge_in_cat(fflat, look, temporal, meas), gamma, beta, eps)


# ----------------------------------------------------------------------------- attention inputs
LATTICE_HW = [(4, 8), (2, 4), (2, 2), (1, 1)]
RANDOM_HW = [(5, 7), (3, 4), (2, 3), (1, 1)]


def lattice_targets(n):
    """The pixel positions the lattice case places on purpose along an axis of n pixels."""
    return [-1.0, -0.5, 0.0, n - 1.0, n - 0.5, float(n), float(n // 2), -64.0, n + 63.0]


def case_logits(R, g):
    """Logits spread to about +-30 (the maximum must be subtracted); head 3 all equal, head 5 one dominant logit."""
    lg = (torch.randn(R, 8, 32, generator=g) * 10).clamp(-30, 30)
    lg[:, 3] = torch.randn(R, 1, generator=g) * 5
    lg[:, 5] = torch.randn(R, 32, generator=g)
    lg[torch.arange(R), 5, torch.arange(R) % 32] += 25.0
    return lg.reshape(R, 256).contiguous()


@functools.lru_cache(maxsize=None)
def lattice_case(B):
    """Power-of-two level sizes, reference points on a 1/64 grid, offsets multiples of 1/8 px: every pixel coordinate is exact
    in f32 and in f64.  Every third row has its reference point on a 1/8 grid and its samples placed at lattice_targets()
    in x and y (all pairs occur).  Head 7 of the last camera samples far outside every map, so its slice of the value
    gradient stays untouched."""
    g = torch.Generator().manual_seed(40 + B)
    BC, R = B * CAMS, B * CAMS * Q
    S = sum(h * w for h, w in LATTICE_HW)
    value = torch.randn(BC, S, 256, generator=g)
    ref = torch.randint(0, 65, (R, 2), generator=g).float() / 64
    off = torch.randint(-24, 25, (R, 8, 4, 8, 2), generator=g).float() / 8
    rows = torch.arange(0, R, 3)
    ref[rows] = torch.randint(0, 9, (rows.numel(), 2), generator=g).float() / 8
    off_far = -70.0                                               # head 7 of the last camera's rows: every sample far outside
    k = (rows.view(-1, 1, 1) // 3 * 64 + torch.arange(8).view(1, 8, 1) * 8 + torch.arange(8).view(1, 1, 8))      # (rows,8,8)
    for lv, (H, W) in enumerate(LATTICE_HW):
        tx, ty = torch.tensor(lattice_targets(W)), torch.tensor(lattice_targets(H))
        n = tx.numel()
        off[rows, :, lv, :, 0] = tx[k % n] + 0.5 - ref[rows, 0].view(-1, 1, 1) * W
        off[rows, :, lv, :, 1] = ty[(k // n + lv) % n] + 0.5 - ref[rows, 1].view(-1, 1, 1) * H
    off[R - Q:, 7] = off_far                                      # ... so that no sample touches (last camera, any position, head 7)
    return dict(level_hw=LATTICE_HW, value=value, offsets=off.reshape(R, 512).contiguous(), logits=case_logits(R, g), ref=ref, B=B)


def integer_band(x):
    """Samples whose float64 pixel coordinate lies within 16 * 2^-24 * max(|x|, 1) of an integer."""
    return (x - x.round()).abs() <= 16 * U32 * x.abs().clamp(min=1.0)


@functools.lru_cache(maxsize=None)
def random_case(B, seed=0):
    """Level sizes neither powers of two nor square, reference points uniform in [-0.1, 1.1], offsets ~ N(0, 2 px); a sample
    whose float64 pixel coordinate is within the integer band is moved by a quarter pixel, so no sample sits where the f32
    and the float64 floor could differ and none is left out of a comparison."""
    g = torch.Generator().manual_seed(1000 * seed + B)
    BC, R = B * CAMS, B * CAMS * Q
    S = sum(h * w for h, w in RANDOM_HW)
    value = torch.randn(BC, S, 256, generator=g)
    ref = torch.rand(R, 2, generator=g) * 1.2 - 0.1
    off = (torch.randn(R, 512, generator=g) * 2).contiguous()
    for _ in range(8):
        x, y = msda_pixels(off.double(), ref.double(), RANDOM_HW)
        near = torch.stack([integer_band(x), integer_band(y)], -1).reshape(R, 512)
        if not bool(near.any()):
            break
        off = torch.where(near, off + 0.25, off)
    return dict(level_hw=RANDOM_HW, value=value, offsets=off, logits=case_logits(R, g), ref=ref.contiguous(), B=B)


def msda_case(name, B):
    return lattice_case(B) if name == "lattice" else random_case(B)


@functools.lru_cache(maxsize=None)
def msda_forward_refs(name, B):
    """(float64 reference, f32 baseline) of msda_ref on a case with f32 values, shared by the tests."""
    c = msda_case(name, B)
    with torch.no_grad():
        r64 = msda_ref(c["value"].double(), c["offsets"].double(), c["logits"].double(), c["ref"].double(), c["level_hw"])
        r32 = msda_ref(c["value"], c["offsets"], c["logits"], c["ref"], c["level_hw"])
    return r64, r32


# ----------------------------------------------------------------------------- query-row inputs
GQ_HW = [(5, 7), (3, 4), (2, 3), (1, 1)]


def hand_made_slots(B):
    """query_of_slot / ref written by hand: -1 pads in the middle and at the end, every point class, heights 0 and 14, reference
    points at 0 and 1, outside the image and at pixel centres, repeated queries."""
    R = B * 4 * 120
    g = torch.Generator().manual_seed(7 + B)
    qos = torch.randint(0, 120, (R,), generator=g, dtype=torch.int32)
    ref = torch.rand(R, 2, generator=g) * 1.4 - 0.2
    qos[3::11] = -1
    qos = qos.reshape(B * 4, 120)
    ref = ref.reshape(B * 4, 120, 2)
    qos[:, 100:] = -1
    qos[:, :16] = torch.tensor([0, 14, 15, 29, 45, 59, 60, 74, 75, 89, 90, 104, 105, 119, 7, 7], dtype=torch.int32)
    corners = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0], [0.5, 0.5], [-0.5, 0.5], [0.5, 1.5], [1.0, 0.25]])
    ref[:, :8] = corners
    qos[0, 5] = -1
    return qos.reshape(B, 4, 120).contiguous(), ref.reshape(B, 4, 120, 2).contiguous()


def gather_inputs(B, g, dt=torch.float64):
    qos, ref = hand_made_slots(B)
    maps = [torch.randn(B * 4, h, w, 256, generator=g).to(dt) for h, w in GQ_HW]
    t = dict(wp=torch.randn(B, 4, 2, generator=g), ctrl=torch.randn(B, 4, 4, generator=g), temporal=torch.randn(4, 128, generator=g),
             static=torch.randn(4, 128, generator=g), meas=torch.randn(B, 128, generator=g), flat=torch.randn(B, 256, generator=g))
    return qos, ref, {k: v.to(dt) for k, v in t.items()}, maps


# ----------------------------------------------------------------------------- LayerNorm of rows that carry an input error
def layernorm_bound_in(x, e, gamma, beta, eps, depth):
    """glue_ref.layernorm_bound for a kernel that normalises rows it has computed itself: x the float64 rows, e >= 0 the bound
    of the kernel's own error on them.  To first order dy_i / dx_j = gamma_i rstd (delta_ij - 1 / D - xh_i xh_j / D), so the
    input error adds |gamma_i| rstd (e_i + mean e + |xh_i| mean(|xh| e)) to the bound of the arithmetic."""
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    e = e.expand_as(x)
    prop = gamma.abs() * rstd * (e + e.mean(1, keepdim=True) + xh.abs() * (xh.abs() * e).mean(1, keepdim=True))
    return layernorm_bound(x, gamma, beta, eps, depth) + prop
