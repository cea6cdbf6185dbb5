"""Float64 references and derived error bounds of the training-step parity tests (test_bn_ops.py, test_dropout_ops.py,
test_optim_ops.py): train-mode BatchNorm forward and backward (csrc/batchnorm.hip), the dropout keep rule, AdamW and the
gradient norm (csrc/optim.hip).  Everything here runs on the CPU and uses no package code; test_step_ref.py pins the references
to torch's float64 operators.

Every bound is a per-element tensor, first order in u = 2^-24 (f32) and w = 2^-53 (f64), obtained by counting the roundings of
the kernel line quoted next to it (glue_ref's rule for reductions: (n + k) u sum|addends|).  A result is an f32 number, so
every bound also carries TINY, the smallest f32 step: it keeps a bound positive where the reference is exactly zero.
"""
import numpy as np
import torch

from glue_ref import U32, sum_bound

U64 = 2.0 ** -53
TINY = 2.0 ** -149
ACT_NONE, ACT_RELU = 0, 1


# ----------------------------------------------------------------------------- BatchNorm
def bn_row_groups(M, groups=1, live=None):
    """[(first row, end row)] of the row groups: `groups` equal parts of M rows, or -- a device row count -- the one group of
    the first min(M, live) rows."""
    if live is not None:
        assert groups == 1
        return [(0, max(0, min(M, int(live))))]
    per = M // groups
    return [(g * per, (g + 1) * per) for g in range(groups)]


def bn_launch_blocks(M, groups=1):
    """bn_rows restated: workgroups per row group, one per 256 allocated rows, between 1 and kBnBlocks = 512."""
    return min(512, max(1, -(-(M // groups) // 256)))


def bn_sum_depth(M, C, groups=1, live=None, vec=False):
    """Additions an addend passes through in the f64 column sums of bn_stats_*_kernel / bn_bwd_reduce_*_kernel followed by
    bn_finish_kernel: a thread adds every TY-th row of its workgroup's ceil(rows / nb) rows (TY = 256 / TX row lanes, TX =
    min(C, 256) channel lanes, C / 4 in the 16-byte kernels), the TY lanes are added in index order, then a slice of
    bn_finish_kernel adds at most ceil(nb / 8) partial rows (its four chains are shorter, + 2 to join them) and the eight
    slices follow.  Never more than the number of rows."""
    nb = bn_launch_blocks(M, groups)
    rows = M // groups if live is None else max(0, min(M, int(live)))
    TX = min((C // 4) if vec else C, 256)
    TY = 256 // TX
    rows_per = -(-rows // nb)
    return max(1, min(rows, -(-rows_per // TY) + TY + -(-nb // 8) + 10))


def _fits_f32(mean, var):
    """bn_finalize_kernel's guard: a statistic that is not finite, or does not fit an f32, must not reach the running buffers."""
    return torch.isfinite(mean) & torch.isfinite(var) & (mean.abs() <= 3.0e38) & (var <= 3.0e38)


def bn_forward_ref(z, gamma, beta, eps, momentum, running_mean, running_var, groups=1, live=None, res=(), act=ACT_NONE):
    """Train-mode BatchNorm of the rows z [M, C] in float64, two-pass variance per group.  gamma / beta / running_*: [C] or None.
    Returns a dict: mean, var (biased), invstd, scale = gamma * invstd [G, C]; out [M, C] = act((z - mean) * scale + beta +
    sum(res)) (rows outside every group: NaN); running_mean / running_var after the groups were applied in index order with
    the unbiased variance (the biased one where a group has a single row; a group without rows, or whose statistic does not
    fit an f32, leaves them alone); n [G]; ez2 = mean z^2 and eabs = mean |z| [G, C] for the bounds."""
    z = z.double()
    M, C = z.shape
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    ga = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    be = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    rm = None if running_mean is None else running_mean.double().clone()
    rv = None if running_var is None else running_var.double().clone()
    rows = bn_row_groups(M, groups, live)
    G = len(rows)
    mean, var, ez2, eabs = (torch.zeros(G, C, dtype=torch.float64) for _ in range(4))
    out = torch.full_like(z, float("nan"))
    rm_steps, rv_steps = [], []                      # (value before, value added) of every applied update, for the bounds
    for g, (a, b) in enumerate(rows):
        n = b - a
        if n > 0:
            zg = z[a:b]
            mean[g] = zg.mean(0)
            var[g] = ((zg - mean[g]) ** 2).mean(0)
            ez2[g], eabs[g] = (zg * zg).mean(0), zg.abs().mean(0)
            unb = var[g] * n / (n - 1.0) if n > 1 else var[g]
            good = _fits_f32(mean[g], var[g])
            if rm is not None:
                rm_steps.append((rm.clone(), mean[g].clone(), good, n))
                rm = torch.where(good, (1.0 - momentum) * rm + momentum * mean[g], rm)
            if rv is not None:
                rv_steps.append((rv.clone(), unb.clone(), good, n))
                rv = torch.where(good, (1.0 - momentum) * rv + momentum * unb, rv)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = ga * invstd
    for g, (a, b) in enumerate(rows):
        if b > a:
            v = (z[a:b] - mean[g]) * scale[g] + be
            for r in res:
                v = v + r.double()[a:b]
            out[a:b] = torch.relu(v) if act == ACT_RELU else v
    return dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=be, out=out, running_mean=rm, running_var=rv,
                n=[b - a for a, b in rows], rows=rows, ez2=ez2, eabs=eabs, gamma=ga, eps=eps, momentum=momentum,
                rm_steps=rm_steps, rv_steps=rv_steps)


def bn_forward_bounds(z, f, res=(), depth=None):
    """Bounds of tt_bn_stats + tt_bn_finalize + tt_bn_apply against bn_forward_ref's dict f.

    Statistics (bn_stats_*_kernel, bn_finish_kernel, bn_finalize_kernel): sum z and sum z^2 in f64 -- the square of an f32 is
    exact in f64 --, each addend through at most d additions (`depth`: bn_sum_depth of the launch; the row count n where it is
    not given), so with E|z|^2 <= E z^2 and |mu| <= E|z|
      mu  = sum z / n                    dmu64  = (d + 1) w E|z|
      var = sum z^2 / n - mu * mu        dvar64 = (d + 1) w E z^2 + (2 (d + 1) + 1) w E z^2 + w var  <=  (3 d + 6) w E z^2
                                         (the one-pass term: relative to E z^2, not to var)
      mean   = (float) mu                                      dmean = u |mu| + dmu64
      invstd = (float) (1 / sqrt(var + eps))                   dis   = invstd (u + dvar64 / (2 (var + eps)) + 3 w)
      scale  = gamma * invstd            one f32 product       dsc   = |gamma| dis + u |scale|
    Apply (bn_apply_*_kernel): v = (z - mean) * scale + shift (+ res1) (+ res2): the subtraction and the product round once
    each (k = 2), then 1 + |res| additions of 2 + |res| addends; the errors of mean and scale enter through their factors:
      dout = |scale| dmean + |z - mean| dsc + sum_bound(|z - mean| |scale| + |shift| + sum |res|, 2 + |res|, 2)
    ReLU is 1-Lipschitz, so the bound holds behind it.
    Running statistics: r' = (1 - m) * r + m * (float) x in f32 -- 1 - m, the two products (or one and an FMA), the sum and
    the cast of x: at most 4 roundings on either addend, two f32 multiply-adds per group; an earlier group's error is
    carried with the factor 1 - m.  x = mu (dmu64) or var n / (n - 1) (dvar64 n / (n - 1) + 2 w x)."""
    z = z.double()
    u, w = U32, U64
    G, C = f["mean"].shape
    nn = torch.tensor([float(n if depth is None else min(n, depth)) for n in f["n"]], dtype=torch.float64).view(G, 1)
    dmu64 = (nn + 1) * w * f["eabs"]
    dvar64 = (3 * nn + 6) * w * f["ez2"]
    dmean = u * f["mean"].abs() + dmu64 + TINY
    dis = f["invstd"] * (u + dvar64 / (2.0 * (f["var"] + f["eps"])) + 3 * w) + TINY
    dsc = f["gamma"].abs() * dis + u * f["scale"].abs() + TINY
    dout = torch.full_like(z, float("nan"))
    for g, (a, b) in enumerate(f["rows"]):
        if b > a:
            d = (z[a:b] - f["mean"][g]).abs()
            s = d * f["scale"][g].abs() + f["shift"].abs()
            for r in res:
                s = s + r.double()[a:b].abs()
            dout[a:b] = f["scale"][g].abs() * dmean[g] + d * dsc[g] + sum_bound(s, 2 + len(res), 2) + TINY
    m = f["momentum"]

    def running(steps, d64_of):
        if not steps:
            return None
        bound = torch.zeros(C, dtype=torch.float64)
        for g, (before, x, good, n) in enumerate(steps):
            step = (1.0 - m) * bound + 4 * u * (((1.0 - m) * before).abs() + (m * x).abs()) + m * d64_of(g, x, n)
            bound = torch.where(good, step, bound)
        return bound + TINY

    live = [g for g in range(G) if f["n"][g] > 0]
    brm = running(f["rm_steps"], lambda i, x, n: dmu64[live[i]])
    brv = running(f["rv_steps"], lambda i, x, n: dvar64[live[i]] * (n / (n - 1.0) if n > 1 else 1.0) + 2 * w * x.abs())
    return dict(mean=dmean, invstd=dis, scale=dsc, out=dout, running_mean=brm, running_var=brv)


def bn_backward_ref(dy, y, z, f, act=ACT_NONE):
    """Backward of bn_forward_ref in float64.  y: the forward's output (its sign decides the ReLU mask; the GPU tests pass the
    values the device wrote, so a result that rounds across zero cannot flip the mask).  Returns g = dy * relu'(y), dres = g,
    the per-group sums sg = sum g and sgx = sum g xhat [G, C], xhat [M, C] and dz = scale (g - sg / n - xhat sgx / n).
    Rows outside every group: g = dy, dz = NaN."""
    dy, z = dy.double(), z.double()
    G, C = f["mean"].shape
    g = dy.clone()
    xh, dz = torch.full_like(z, float("nan")), torch.full_like(z, float("nan"))
    sg, sgx = torch.zeros(G, C, dtype=torch.float64), torch.zeros(G, C, dtype=torch.float64)
    for i, (a, b) in enumerate(f["rows"]):
        if b > a:
            n = b - a
            if act == ACT_RELU:
                g[a:b] = torch.where(y[a:b] > 0, dy[a:b], torch.zeros_like(dy[a:b]))
            xh[a:b] = (z[a:b] - f["mean"][i]) * f["invstd"][i]
            sg[i], sgx[i] = g[a:b].sum(0), (g[a:b] * xh[a:b]).sum(0)
            dz[a:b] = f["scale"][i] * (g[a:b] - sg[i] / n - xh[a:b] * sgx[i] / n)
    return dict(g=g, dres=g, sg=sg, sgx=sgx, xhat=xh, dz=dz)


def bn_backward_bounds(z, f, fb, b, depth=None):
    """Bounds of tt_bn_bwd_reduce + tt_bn_bwd_apply against bn_backward_ref's dict b (f, fb: the forward's reference and bounds).

      xh  = (z - mean) * invstd   f32: subtraction, product          dxh  = invstd (u |z - mean| + dmean) + |z - mean| dis + u |xhat|
      sg  = sum g                 f64 sum of f32 values               dsg  = d w sum |g|      (d: `depth`, as in bn_forward_bounds)
      sgx = sum g * xh            f64: the product of two f32 is exact   dsgx = d w sum |g xhat| + sum |g| dxh
    (dgamma / dbeta are these sums: f64 sums of f32 terms.)
      A = (float) sg * (float) (1 / n), B likewise   three roundings    dA = 3 u |A| + dsg / n,  dB = 3 u |B| + dsgx / n
      dz = scale * (g - A - xh * B)   the product xh * B and the one with scale (k = 2), two subtractions of three addends:
      ddz = |scale| (sum_bound(|g| + |A| + |xhat B|, 3, 2) + dA + |xhat| dB + dxh |B|) + dsc |g - A - xhat B|"""
    z = z.double()
    u, w = U32, U64
    G, C = f["mean"].shape
    dsg, dsgx = torch.zeros(G, C, dtype=torch.float64), torch.zeros(G, C, dtype=torch.float64)
    ddz = torch.full_like(z, float("nan"))
    for i, (a, e) in enumerate(f["rows"]):
        if e > a:
            n = e - a
            d = (z[a:e] - f["mean"][i]).abs()
            g, xh = b["g"][a:e], b["xhat"][a:e]
            dxh = f["invstd"][i] * (u * d + fb["mean"][i]) + d * fb["invstd"][i] + u * xh.abs()
            dd = n if depth is None else min(n, depth)
            dsg[i] = dd * w * g.abs().sum(0)
            dsgx[i] = dd * w * (g * xh).abs().sum(0) + (g.abs() * dxh).sum(0)
            A, B = b["sg"][i] / n, b["sgx"][i] / n
            dA, dB = 3 * u * A.abs() + dsg[i] / n, 3 * u * B.abs() + dsgx[i] / n
            inner = g - A - xh * B
            ddz[a:e] = (f["scale"][i].abs() * (sum_bound(g.abs() + A.abs() + (xh * B).abs(), 3, 2) + dA + xh.abs() * dB + dxh * B.abs())
                        + fb["scale"][i] * inner.abs() + TINY)
    return dict(sg=dsg + TINY, sgx=dsgx + TINY, dz=ddz)


# ----------------------------------------------------------------------------- dropout
def dropout_keep_ref(seed, n, p):
    """dropout_fwd_kernel's keep rule: splitmix64(seed + golden * (i + 1)), its top 24 bits as an f32 times 2^-24 -- both
    exact --, kept when >= (float) p.  Returns a uint8 numpy array of n keep flags."""
    with np.errstate(over="ignore"):
        i = np.arange(1, n + 1, dtype=np.uint64)
        zz = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + np.uint64(0x9E3779B97F4A7C15) * i
        zz = (zz ^ (zz >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        zz = (zz ^ (zz >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        zz = zz ^ (zz >> np.uint64(31))
    r = (zz >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    return (r >= np.float32(p)).astype(np.uint8)


def dropout_seed_drawing(u24, index, low=0x123456789A):
    """A seed under which element `index` draws exactly u24 * 2^-24: splitmix64 is a bijection, so its finalizer is inverted
    from a hash whose top 24 bits are u24 (`low`: the 40 bits below them).  With u24 * 2^-24 == (float) p this is the edge of
    the keep rule, which a mask of random draws meets once in 2^24 elements."""
    mask = 0xFFFFFFFFFFFFFFFF
    zz = ((u24 & 0xFFFFFF) << 40) | (low & 0xFFFFFFFFFF)
    zz ^= zz >> 31
    zz ^= zz >> 62
    zz = (zz * pow(0x94D049BB133111EB, -1, 1 << 64)) & mask
    zz ^= zz >> 27
    zz ^= zz >> 54
    zz = (zz * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & mask
    zz ^= zz >> 30
    zz ^= zz >> 60
    return (zz - 0x9E3779B97F4A7C15 * (index + 1)) & mask


def dropout_inv_keep(p):
    """(float) 1 / (1 - p) as the kernel forms it: both f32 operations are correctly rounded."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


# ----------------------------------------------------------------------------- AdamW and the gradient norm
def f32r(x):
    """A hyper-parameter as the C ABI receives it: rounded to f32."""
    return float(np.float32(x))


def adamw_ref(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale=None, round_hyper=True):
    """One AdamW update (torch.optim.AdamW's formulation) in float64; `step` is the 1-based count of this update.  With
    round_hyper the hyper-parameters are rounded to f32 first (1 - 0.999f is not torch's 1 - 0.999).  Returns p, m, v."""
    if round_hyper:
        lr, beta1, beta2, eps, weight_decay = (f32r(t) for t in (lr, beta1, beta2, eps, weight_decay))
        grad_scale = None if grad_scale is None else f32r(grad_scale)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gi = g if grad_scale is None else g * grad_scale
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p = p * (1.0 - lr * weight_decay)
    m = m + (gi - m) * (1.0 - beta1)
    v = v * beta2 + gi * gi * (1.0 - beta2)
    denom = v.sqrt() / bc2 ** 0.5 + eps
    return p - (lr / bc1) * (m / denom), m, v


def adamw_bounds(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale=None):
    """Bounds (bp, bm, bv) of adamw_kernel / adamw_dev_step_kernel against adamw_ref on the same inputs, counted on

      gi = g * gs                                   one product with a clip factor, none without    dgi = kg u |gi|
      mi = m + (gi - m) * (1 - beta1)               subtraction, the constant, product, sum (1 - beta1 is exact for
                                                    beta1 in [0.5, 1), counted all the same)
                                                                                     dm = c1 dgi + 3 u c1 |gi - m| + u |mi|
      vi = v * beta2 + gi * gi * (1 - beta2)        square, constant, product | product | sum
                                                                     dv = 2 c2 |gi| dgi + 3 u c2 gi^2 + u beta2 v + u vi
      denom = sqrtf(vi) / bc2s + eps                root, the f32 cast of bc2s, quotient, sum
                                               dden = (dv / (2 sqrt vi) + 3 u sqrt vi) / bc2s + u denom   (vi = 0: exactly eps)
      q = mi / denom                                                              dq = dm / denom + |q| dden / denom + u |q|
      pi = p * (1 - lr * wd) - (lr / bc1) * q       lr * wd, 1 - ., product: 3 on |p|; the cast of bc1, lr / bc1, the product
                                                    with q: 3 on the step; the subtraction on the result
                                                            dp = 3 u |p| + (lr / bc1) (dq + 3 u |q|) + u |pi|
    The device's f64 pow and sqrt of the bias corrections are within a few w of the reference's: inside the cast's u."""
    u = U32
    lr, beta1, beta2, eps, weight_decay = (f32r(t) for t in (lr, beta1, beta2, eps, weight_decay))
    gs = None if grad_scale is None else f32r(grad_scale)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    pn, mn, vn = adamw_ref(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, gs, round_hyper=False)
    gi = g if gs is None else g * gs
    c1, c2 = 1.0 - beta1, 1.0 - beta2
    bc1, bc2s = 1.0 - beta1 ** step, (1.0 - beta2 ** step) ** 0.5
    dgi = (0.0 if gs is None else u) * gi.abs()
    dm = c1 * dgi + 3 * u * c1 * (gi - m).abs() + u * mn.abs()
    dv = 2 * c2 * gi.abs() * dgi + 3 * u * c2 * gi * gi + u * beta2 * v.abs() + u * vn.abs()
    rt = vn.sqrt()
    drt = torch.where(rt > 0, dv / (2.0 * rt.clamp_min(1e-300)), torch.zeros_like(rt))
    denom = rt / bc2s + eps
    dden = (drt + 3 * u * rt) / bc2s + u * denom
    q = mn / denom
    dq = dm / denom + q.abs() * dden / denom + u * q.abs()
    dp = 3 * u * p.abs() + (lr / bc1) * (dq + 3 * u * q.abs()) + u * pn.abs()
    return dp + TINY, dm + TINY, dv + TINY


def grad_norm_ref(g):
    """The float64 L2 norm."""
    return float(g.double().pow(2).sum().sqrt())


def grad_norm_bound(g, blocks=None):
    """Bound of tt_grad_norm_clip's norm.  sumsq_partial_kernel: min(1024, ceil(n / 256)) blocks of 256 threads, a thread adds
    d = ceil(n / (blocks * 256)) squares in f32 (the square rounds once), then the 8-level f32 tree over the 256 threads:
    sum_bound(sum g^2, d + 8, 1).  norm_finalize_kernel adds the partials, takes the root in f64 and casts:
      dnorm = dS / (2 norm) + u norm."""
    n = g.numel()
    blocks = blocks or min(1024, -(-n // 256))
    d = -(-n // (blocks * 256))
    S = float(g.double().pow(2).sum())
    norm = S ** 0.5
    return (sum_bound(S, d + 8, 1) / (2.0 * norm) if norm > 0 else 0.0) + U32 * norm + TINY


def clip_factor_ref(norm_f32, max_norm):
    """min(1, max_norm / (norm + 1e-6f)) in f32 from the f32 norm the kernel returned: two correctly rounded operations."""
    coef = np.float32(max_norm) / (np.float32(norm_f32) + np.float32(1e-6))
    return np.float32(coef if coef < np.float32(1.0) else 1.0)


# ----------------------------------------------------------------------------- the BatchNorm case list (GPU tests and CPU pin)
class BnCase:
    """One BatchNorm parity case.  data: 'randn' (columns of varied offset and spread), 'cond' (column 0 = 100 + 0.01 randn),
    'const' (column 0 exactly constant), 'huge' (column 0 ~ 1e18: its squares only fit f64), 'bad' (a NaN in column 2, an
    overflowed 3e38 * 2 in column 5).  lay: 'win' (every tensor in its own channel window) or
    (tensor, how) -- all aligned windows but `tensor`, which is `shift`ed one float past a 16-byte boundary or given an
    odd `coff` / `cstride`.  live: the device row count (None: dense groups)."""

    def __init__(self, cid, M, C, groups=1, act=ACT_NONE, nres=0, live=None, data="randn", gamma=True, beta=True, running=True,
                 momentum=0.1, lay="win", arm=None):
        self.id, self.M, self.C, self.groups, self.act, self.nres, self.live, self.data = cid, M, C, groups, act, nres, live, data
        self.gamma, self.beta, self.running, self.momentum, self.lay, self.arm = gamma, beta, running, momentum, lay, arm
        self.eps = 1e-5

    def __repr__(self):
        return self.id


def bn_case_data(c):
    """The f32 host tensors of a case: z [M, C], gamma, beta, running_mean, running_var [C] (None where the case has none),
    res (list of [M, C]), dy [M, C] with |dy| <= 8 (inside the gradient prefill's ulp)."""
    gen = torch.Generator().manual_seed(1000 * c.C + c.M % 9973 + 17 * c.groups + c.nres)
    M, C = c.M, c.C
    z = torch.randn(M, C, generator=gen) * (torch.rand(1, C, generator=gen) * 3 + 0.2) + torch.randn(1, C, generator=gen) * 2
    if c.data == "cond":
        z[:, 0] = 100.0 + 0.01 * torch.randn(M, generator=gen)
    elif c.data == "const":
        z[:, 0] = 0.3                                   # f32(0.3): 24 significant bits
    elif c.data == "huge":
        z[:, 0] = 1e18 * (1.0 + torch.randn(M, generator=gen))
    elif c.data == "bad":
        z[M // 3, 2] = float("nan")
        z[M // 2, 5] = torch.tensor(3e38) * 2
    if c.live is not None:
        z[max(0, min(M, c.live)):] = 1e6
    gamma = (torch.randn(C, generator=gen) * 0.5 + 1.0) if c.gamma else None
    beta = torch.randn(C, generator=gen) if c.beta else None
    rm = torch.randn(C, generator=gen) if c.running else None
    rv = (torch.rand(C, generator=gen) + 0.5) if c.running else None
    res = [torch.randn(M, C, generator=gen) for _ in range(c.nres)]
    dy = torch.randn(M, C, generator=gen).clamp(-7.0, 7.0)
    return dict(z=z, gamma=gamma, beta=beta, rm=rm, rv=rv, res=res, dy=dy)


def _bn_cases():
    R = ACT_RELU
    cs = []
    # scalar arm by channel count (257 > 256: two trips of the scalar channel loop)
    for i, C in enumerate((1, 3, 22, 257)):
        cs.append(BnCase(f"scalar-C{C}-g1-none-res{i % 3}", 70, C, 1, ACT_NONE, i % 3, arm="scalar"))
        cs.append(BnCase(f"scalar-C{C}-g2-relu-res{(i + 1) % 3}", 140, C, 2, R, (i + 1) % 3, arm="scalar"))
    # scalar arm by alignment: one tensor off at a time
    for t, how2 in (("z", "coff"), ("out", "cstride"), ("res1", "coff"), ("dy", "cstride"), ("y", "coff"), ("dres1", "cstride"),
                    ("dz", "coff")):
        for how in ("shift", how2):
            cs.append(BnCase(f"misaligned-{t}-{how}", 70, 8, 1, R, 1, lay=(t, how), arm="mixed"))
    # vector arm (1028 > 1024: two trips of the vector tile loop; 12, 300: TX does not divide 256)
    for i, C in enumerate((4, 12, 300, 1028)):
        cs.append(BnCase(f"vector-C{C}-g1-relu-res{i % 3}", 70, C, 1, R, i % 3, arm="vec"))
        cs.append(BnCase(f"vector-C{C}-g2-none-res{(i + 2) % 3}", 140, C, 2, ACT_NONE, (i + 2) % 3, arm="vec"))
    # rows per group: nb = 1, 2, >= 25 (the four-chain loop of bn_finish_kernel), a remainder in it, the 512 clamp
    for rows in (1, 2, 255, 256, 257, 6145, 8 * 256 * 4 + 1, 131072 + 257):
        cs.append(BnCase(f"rows{rows}-C4", rows, 4, 1, R, 1, arm="vec"))
        cs.append(BnCase(f"rows{rows}-C3", rows, 3, 1, R, 1, arm="scalar"))
    cs.append(BnCase("rows6145x3groups-C4", 3 * 6145, 4, 3, ACT_NONE, 0, arm="vec"))
    cs.append(BnCase("rows6145x3groups-C3", 3 * 6145, 3, 3, ACT_NONE, 0, arm="scalar"))
    # device row count
    for C, arm in ((6, "scalar"), (48, "vec")):
        for live in (0, 1, 37, 4321, 5000, 7000):
            cs.append(BnCase(f"live{live}-of-5000-C{C}", 5000, C, 1, R, 1, live=live, arm=arm))
    # finalize
    cs.append(BnCase("null-gamma", 70, 8, 1, ACT_NONE, 0, gamma=False, arm="vec"))
    cs.append(BnCase("null-beta", 70, 8, 1, ACT_NONE, 0, beta=False, arm="vec"))
    cs.append(BnCase("null-running", 70, 8, 1, ACT_NONE, 0, running=False, arm="vec"))
    cs.append(BnCase("non-finite-channels", 70, 8, 1, ACT_NONE, 0, data="bad", arm="vec"))
    cs.append(BnCase("g2-momentum0.01", 140, 8, 2, ACT_NONE, 0, momentum=0.01, arm="vec"))
    cs.append(BnCase("g2-momentum1.0", 140, 8, 2, ACT_NONE, 0, momentum=1.0, arm="vec"))
    # conditioning
    cs.append(BnCase("cond-mean100-dev0.01", 6400, 4, 1, ACT_NONE, 0, data="cond", arm="vec"))
    cs.append(BnCase("constant-column", 6400, 4, 1, ACT_NONE, 0, data="const", arm="vec"))
    cs.append(BnCase("constant-column-C3", 300, 3, 1, ACT_NONE, 0, data="const", arm="scalar"))
    cs.append(BnCase("huge-1e18", 6400, 4, 1, ACT_NONE, 0, data="huge", arm="vec"))
    return cs


BN_CASES = _bn_cases()
DROPOUT_SEEDS = (0, 0x5EED, 2 ** 64 - 1)
DROPOUT_PS = (0.0, 0.1, 0.5, 0.9)
# (p, u24) with u24 * 2^-24 == (float) p: 0 and 0.5 trivially, (float) 0.9 = 15099494 * 2^-24 ((float) 0.1 is off that grid)
DROPOUT_EDGES = ((0.0, 0), (0.5, 1 << 23), (0.9, 15099494))
