"""Float64 references, error bounds and buffer helpers of the glue-kernel parity tests (test_glue_ops.py, test_glue_bwd.py).

Everything here runs on the CPU.  The references torch does not already provide are restated in float64 (lift-splat, the
deformable columns with their corner values, the first-maximum max-pool backward, the integer nearest rule); the tolerance
helpers implement the two rules of the tests:

  * elementwise / interpolating kernels: 4 x the error of torch's own f32 CPU evaluation of the same expression against the
    float64 reference on the same inputs, and never less than 8 * 2^-24 (`f32_limit`), relative to max|ref|;
  * reductions: the classical recursive-summation bound (n + k) * 2^-24 * sum|addends| per element (`sum_bound`), n the
    number of addends and k the roundings before and after the sum, counted from the kernel next to each case;
  * 16-bit storage adds one storage ulp of |ref| (2^-8 bf16, 2^-11 f16).

`check` / `check_equal` print the measured error and the limit of every comparison and keep the worst per kernel; with
TT_GLUE_PARITY_OUT=<file> the per-kernel table is written there when the process ends (profiles/glue_ops_parity.txt).
"""
import atexit
import os

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                    # unit roundoff of f32
STORE_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SENT = -1234.5                      # sentinel of the guard rows / columns (exact in f32, bf16-rounded on 16-bit buffers)
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_GELU, ACT_SOFTPLUS, ACT_SOFTPLUS_CLAMP = range(6)
ACT_NAMES = {0: "none", 1: "relu", 2: "sigmoid", 3: "gelu", 4: "softplus", 5: "softplus_clamp"}


# ----------------------------------------------------------------------------- tolerances and the report
def sum_bound(abs_addends_sum, n, k):
    """(n + k) * 2^-24 * sum|addends|: error bound of an n-term f32 recursive sum with k further roundings."""
    return (n + k) * U32 * abs_addends_sum


def rel_err(got, ref):
    ref = ref.double()
    scale = float(ref.abs().max())
    return float((got.double() - ref).abs().max()) / (scale if scale > 0 else 1.0)


def f32_limit(r32, r64):
    """The elementwise rule: max(4 x torch-f32's own error against float64, 8 * 2^-24), relative to max|ref|."""
    return max(4.0 * rel_err(r32, r64), 8.0 * U32)


_WORST = {}


def _record(kernel, case, err, lim, note=""):
    print(f"PARITY {kernel:28s} {case:44s} err {err:.3e}  limit {lim:.3e} {note}")
    _record_file()
    w = _WORST.get(kernel)
    ratio = err / lim if lim > 0 else 0.0
    n = (w[5] if w else 0) + 1
    if w is None or ratio > w[0] or (ratio == w[0] and lim > w[2]):
        _WORST[kernel] = (ratio, err, lim, case, note, n)
    else:
        _WORST[kernel] = w[:5] + (n,)


def check(kernel, case, got, ref, rel=0.0, bound=None, store=torch.float32, slack=0.0):
    """|got - ref| <= rel * max|ref| + bound + store_ulp * |ref| + slack, elementwise.  `rel` is the per-tensor relative limit,
    `bound` a per-element absolute one (a summation bound), `slack` the accumulation allowance (1 ulp of the prefill).
    Reported: the largest error (or the one furthest over its limit) and the limit at that element, both over max|ref|."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (kernel, case, got.shape, ref.shape)
    scale = float(ref.abs().max()) if ref.numel() else 1.0
    scale = scale if scale > 0 else 1.0
    lim = torch.full_like(ref, rel * scale + slack) + STORE_ULP[store] * ref.abs()
    if bound is not None:
        lim = lim + bound
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.where(got == ref, torch.zeros_like(err), torch.full_like(err, float("inf"))), err)
    if err.numel() == 0:
        return
    i = int(err.reshape(-1).argmax())                 # reported: the largest error, or the first one over its limit
    if not bool((err <= lim).all()):
        i = int((err - lim).reshape(-1).argmax())
    _record(kernel, case, float(err.reshape(-1)[i]) / scale, float(lim.reshape(-1)[i]) / scale)
    assert bool((err <= lim).all()), (f"{kernel} [{case}]: error {float(err.reshape(-1)[i]):.3e} over its limit "
                                      f"{float(lim.reshape(-1)[i]):.3e} at flat index {i} (max|ref| {scale:.3e})")


def check_equal(kernel, case, got, want):
    """Bit-equal (data movement and single-rounding ops)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (kernel, case, got.shape, want.shape, got.dtype, want.dtype)
    same = torch.equal(got, want)
    _record(kernel, case, 0.0 if same else float("inf"), 0.0, "bit-equal")
    assert same, f"{kernel} [{case}]: not bit-equal to torch ({int((got != want).sum())} of {got.numel()} elements differ)"


_FILES = set()


def _record_file():
    """The test file whose check is being recorded (the table's header names the files that were actually run)."""
    cur = os.environ.get("PYTEST_CURRENT_TEST", "")
    if cur:
        _FILES.add(cur.split("::")[0])


def _write_table():
    path = os.environ.get("TT_GLUE_PARITY_OUT")
    if not path or not _WORST:
        return
    files = " ".join(sorted(_FILES)) or "<no test file>"
    with open(path, "w") as f:
        f.write("# worst measured error of every kernel checked and the limit it was held to (both relative to max|ref64| of the\n"
                "# output tensor; `bit-equal`: compared with torch.equal), over all cases of the test files run.  Produced by\n"
                f"#   TT_GLUE_PARITY_OUT={path} python -m pytest {files} -m gpu -q\n"
                f"# {'kernel':28s} {'checks':>6s} {'worst err':>10s} {'its limit':>10s}  case\n")
        for k in sorted(_WORST):
            ratio, err, lim, case, note, n = _WORST[k]
            f.write(f"{k:30s} {n:6d} {err:10.3e} {lim:10.3e}  {case} {note}\n")


atexit.register(_write_table)


# ----------------------------------------------------------------------------- guarded buffers
class Win:
    """A device buffer of R rows x `cstride` columns plus `guard` extra rows, all sentinel (or `prefill`), whose channel
    window [coff, coff + C) of the first R rows is what a kernel may write.  `untouched()` asserts the rest bit-unchanged."""

    def __init__(self, R, C, cstride=None, coff=0, dtype=torch.float32, init=None, guard=2):
        self.R, self.C, self.cs, self.coff = R, C, cstride or C, coff
        host = torch.full((R + guard, self.cs), SENT).to(dtype)
        if init is not None:
            host[:R, coff:coff + C] = init.reshape(R, C).to(dtype)
        self.host0 = host.clone()
        self.buf = host.cuda()

    def ptr(self):                      # row 0, column 0: for entry points that take (stride, coff)
        return self.buf.data_ptr()

    def wptr(self):                     # row 0, column coff: for entry points that take a stride only
        return self.buf.data_ptr() + self.coff * self.buf.element_size()

    def get(self):                      # the window, on the host, in the buffer's dtype
        return self.buf.cpu()[:self.R, self.coff:self.coff + self.C].contiguous()

    def init(self):
        return self.host0[:self.R, self.coff:self.coff + self.C].contiguous()

    def untouched(self, what=""):
        now = self.buf.cpu()
        m = torch.ones(now.shape, dtype=torch.bool)
        m[:self.R, self.coff:self.coff + self.C] = False
        assert torch.equal(now[m], self.host0[m]), f"{what}: wrote outside its window / rows"


def prefill(shape, gen):
    """Gradient-destination pattern: |P| in [8, 16) with random sign, so one ulp of every element is 2^-20 and the rounding of
    P + g (|g| <= 8) is within it.  PREFILL_ULP is the accumulation slack of the tests."""
    return (8.0 + 8.0 * torch.rand(shape, generator=gen)) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()


PREFILL_ULP = 2.0 ** -20


# ----------------------------------------------------------------------------- references torch does not provide
def act_ref(v, act):
    if act == ACT_NONE:
        return v
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    if act == ACT_GELU:
        return F.gelu(v)
    if act == ACT_SOFTPLUS:
        return F.softplus(v)
    if act == ACT_SOFTPLUS_CLAMP:
        return F.softplus(v).clamp(min=1e-3)
    raise ValueError(act)


def nearest_index(n_out, n_in):
    """The integer nearest rule of tt_upsample_nearest_add: source index floor(y * h / H)."""
    return (torch.arange(n_out) * n_in) // n_out


def nearest_up(src, H, W):
    """src [N,h,w,C] -> [N,H,W,C] by the integer rule (differentiable: index_select)."""
    return src.index_select(1, nearest_index(H, src.shape[1])).index_select(2, nearest_index(W, src.shape[2]))


def maxpool3x3s2_bwd_first_max(x, dy):
    """Literal F.max_pool2d(x, 3, 2, 1) backward on channel-last x [N,H,W,C]: the gradient of every window goes to its FIRST
    maximum in (kh, kw) scan order."""
    N, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dx = torch.zeros_like(x)
    for n in range(N):
        for oh in range(OH):
            for ow in range(OW):
                for c in range(C):
                    best, arg = None, None
                    for dh in range(3):
                        for dw in range(3):
                            yy, xx = 2 * oh - 1 + dh, 2 * ow - 1 + dw
                            if 0 <= yy < H and 0 <= xx < W and (arg is None or x[n, yy, xx, c] > best):
                                best, arg = x[n, yy, xx, c], (yy, xx)
                    dx[n, arg[0], arg[1], c] += dy[n, oh, ow, c]
    return dx


def lift_splat_ref(logits, ctx, geom, voxel_num, B, ncam):
    """softmax(logits) (x) ctx scattered into the BEV cells.  logits [B*ncam,fH,fW,D], ctx [B*ncam,fH,fW,C] (float64,
    differentiable), geom int [B, ncam*D*fH*fW, 3] in (cam, d, h, w) order -> [B,Y,X,C]; a point with any coordinate out of
    range is dropped."""
    X, Y, Z = voxel_num
    BN, fH, fW, D = logits.shape
    C = ctx.shape[-1]
    p = logits.softmax(-1)                                                    # [BN,fH,fW,D]
    vol = p.permute(0, 3, 1, 2).unsqueeze(-1) * ctx.unsqueeze(1)              # [BN,D,fH,fW,C]
    vol = vol.reshape(B, ncam * D * fH * fW, C)
    g = geom.long()
    ok = ((g[..., 0] >= 0) & (g[..., 0] < X) & (g[..., 1] >= 0) & (g[..., 1] < Y) & (g[..., 2] >= 0) & (g[..., 2] < Z))
    out = torch.zeros(B * Y * X, C, dtype=logits.dtype)
    cell = (torch.arange(B).view(B, 1) * Y + g[..., 1]) * X + g[..., 0]
    return out.index_add(0, cell[ok], vol[ok]).reshape(B, Y, X, C)


def im2col3x3_zero_pad(x):
    """x [N,H,W,C] -> [N*H*W, 9, C]: the plain zero-padded 3 x 3 columns (tap = 3 * kh + kw)."""
    N, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return torch.stack([xp[:, i:i + H, j:j + W] for i in range(3) for j in range(3)], 3).reshape(N * H * W, 9, C)


def deform_sample(x, off, pad=1):
    """The sampling geometry of tt_deform_im2col3x3 in float64, from f32 inputs: x [N,H,W,C], off [N,H,W,>=18] ->
    dict(py, px [N,H,W,9], w [N,H,W,9,4] corner weights (0 where the corner is outside), a [N,H,W,9,4,C] corner values,
    idx [N,H,W,9,4] flat pixel index of the corner (clamped), valid [N,H,W,9,4])."""
    N, H, W, C = x.shape
    x, off = x.double(), off.double()
    tap = torch.arange(9)
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1, 1) + (tap // 3 - pad).view(1, 1, 1, 9)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W, 1) + (tap % 3 - pad).view(1, 1, 1, 9)
    py, px = ys + off[..., 0:18:2], xs + off[..., 1:18:2]
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    y0, x0 = torch.floor(py), torch.floor(px)
    ly, lx = py - y0, px - x0
    cy = torch.stack([y0, y0, y0 + 1, y0 + 1], -1).long()
    cx = torch.stack([x0, x0 + 1, x0, x0 + 1], -1).long()
    w = torch.stack([(1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx], -1)
    valid = inside.unsqueeze(-1) & (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
    idx = (torch.arange(N).view(N, 1, 1, 1, 1) * H + cy.clamp(0, H - 1)) * W + cx.clamp(0, W - 1)
    a = x.reshape(N * H * W, C)[idx] * valid.unsqueeze(-1)
    return dict(py=py, px=px, ly=ly, lx=lx, w=w * valid, a=a, idx=idx, valid=valid, inside=inside)


def deform_cols(x, off, pad=1):
    """float64 deformable columns [N*H*W, 9, C] from the corner restatement (checked against oracle.model_ref.deform_im2col)."""
    s = deform_sample(x, off, pad)
    N, H, W, C = x.shape
    return (s["w"].unsqueeze(-1) * s["a"]).sum(4).reshape(N * H * W, 9, C)


# ----------------------------------------------------------------------------- LayerNorm: data and error bounds
def wave_sum_depth(n):
    """Additions an addend passes through when one 64-lane wave sums n elements: ceil(n / 64) per lane, six butterfly steps
    (never more than n: adding the zeros of idle lanes is exact)."""
    return min(n, -(-n // 64) + 6)


def ln_rows(R, D, gen):
    """Rows of varied scale and offset; row 0 constant (variance 0), row 1 with mean 1e3 and unit spread."""
    x = torch.randn(R, D, generator=gen) * (torch.rand(R, 1, generator=gen) * 3 + 0.2) + torch.randn(R, 1, generator=gen)
    x[0] = 0.75
    if R > 1:
        x[1] = 1e3 + torch.randn(D, generator=gen)
    return x


def _ln_terms(x, eps, depth=None):
    """Float64 statistics of the rows of x and the first-order error of their f32 evaluation (u = 2^-24).  A row is summed by
    one wave: every lane adds ceil(D / 64) elements, then six butterfly steps, so no addend passes through more than
    h = ceil(D / 64) + 6 additions; the summation bound holds with h in the place of the number of addends (and is 25 x
    tighter at D = 256, which matters for the row with mean 1e3).
      mean : h additions + the division               dm   = (h + 1) u mean|x|
      d    : x - mean, one rounding                   dd   = dm + u |d|
      var  : h additions of d^2 (+ square, division)  dvar = (h + 3) u var + mean(2 |d| dd + dd^2)
      rstd : add eps, sqrt, reciprocal (relative)     dr   = 0.5 dvar / (var + eps) + 3 u
      xh   : d * rstd                                 dxh  = rstd dd + |xh| (dr + u)
    `depth` replaces h for a kernel that sums its rows another way (counted next to the case that passes it)."""
    u, h = U32, (wave_sum_depth(x.shape[1]) if depth is None else depth)
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    dm = (h + 1) * u * x.abs().mean(1, keepdim=True)
    dd = dm + u * d.abs()
    dvar = (h + 3) * u * var + (2 * d.abs() * dd + dd * dd).mean(1, keepdim=True)
    dr = 0.5 * dvar / (var + eps) + 3 * u
    xh = d * rstd
    return d, rstd, dd, dr, xh, rstd * dd + xh.abs() * (dr + u)


def layernorm_bound(x, gamma, beta, eps, depth=None):
    """Per-element bound of y = (x - mean) * rstd * gamma + beta in f32: |gamma| dxh + 3 u (|xh gamma| + |y|) (two products, one add)."""
    d, rstd, dd, dr, xh, dxh = _ln_terms(x, eps, depth)
    y = xh * gamma + beta
    return gamma.abs() * dxh + 3 * U32 * ((xh * gamma).abs() + y.abs())


def layernorm_bwd_bounds(x, gamma, g, eps, chain):
    """Bounds of tt_layernorm_rows_bwd's outputs: dx = rstd (gg - a - xh b), gg = g gamma, a = mean gg, b = mean(gg xh);
    dgamma = sum_rows g xh, dbeta = sum_rows g, the column sums along a chain of `chain` additions (rows of a block, then blocks).
      a  : h additions, the product, the division     da = (h + 2) u mean|gg|        (h as in _ln_terms)
      b  : h additions, two products, the division    db = (h + 3) u mean|gg xh| + mean(|gg| dxh)
      dx : rstd (u |gg| + da + |xh| db + |b| dxh) + (dr + 4 u) rstd (|gg| + |a| + |xh b|)"""
    u, h = U32, wave_sum_depth(x.shape[1])
    d, rstd, dd, dr, xh, dxh = _ln_terms(x, eps)
    gg = g * gamma
    a, b = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    da = (h + 2) * u * gg.abs().mean(1, keepdim=True)
    db = (h + 3) * u * (gg * xh).abs().mean(1, keepdim=True) + (gg.abs() * dxh).mean(1, keepdim=True)
    bdx = rstd * (u * gg.abs() + da + xh.abs() * db + b.abs() * dxh) + (dr + 4 * u) * rstd * (gg.abs() + a.abs() + (xh * b).abs())
    bdg = sum_bound((g * xh).abs().sum(0), chain, 1) + (g.abs() * dxh).sum(0)
    bdb = sum_bound(g.abs().sum(0), chain, 0)
    return bdx, bdg, bdb


# ----------------------------------------------------------------------------- backward plumbing
def vjp(fn, xs, dy, dtype=torch.float64):
    """Gradients of fn(*xs) against the cotangent dy, by torch autograd in `dtype` (float64: the reference; float32: the baseline)."""
    leaves = [x.to(dtype).clone().requires_grad_(True) for x in xs]
    fn(*leaves).backward(dy.to(dtype))
    return [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaves]


def fit_scale(*refs):
    """A power of two s with s * max|ref| <= 4: the cotangent of a backward test is scaled by it (exactly), so every gradient
    stays below the prefill's magnitude and the rounding of prefill + gradient is within one ulp of the prefill."""
    m = max(float(r.abs().max()) for r in refs)
    s = 1.0
    while m * s > 4.0:
        s *= 0.5
    return s
