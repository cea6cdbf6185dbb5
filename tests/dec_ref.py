"""Float64 references, bf16x3 emulation, limits and cases of the decoder's spatial kernels and row chains
(csrc/dec_spatial.hip: tt_dec_gru, tt_dec_flatten, tt_dec_bev_update; csrc/dec_chain.hip: tt_mlp_chain, tt_mlp_chain_wide).
Used by test_dec_ref.py (CPU) and test_dec_ops.py (GPU).  Everything here runs on the CPU.

Each of the four operations is written ONCE, from the reference formulas the kernel comments cite, over an arithmetic `A`:

  * `F64` / `F32`: plain torch in that precision -- the float64 restatement (the reference) and torch's own f32 evaluation;
  * `X3()`: the arithmetic the kernels promise (csrc/bf16x3.h).  Before every convolution or linear layer the activations and the
    weights are split, hi = rne_bf16(x), lo = rne_bf16(x - hi); the three partial products hi*hi, hi*lo, lo*hi are three torch f32
    convolutions / matmuls added in f32.  Everything else is f32: biases, the constant-input term of the GRU, activations, the
    blend, BatchNorm.  One thing is added to that, read from the kernels: a value that a kernel keeps in a pair-format LDS map and
    reads back OUTSIDE a convolution is hi + lo there, not the f32 value (`hold`): the GRU state in the blend (Smap), and on the
    10 x 10 level of grid2feat the conv21_10 output in the SE block's residual, MLP10's y in its pooling and gating, and the
    block output (the `mids` copy is a pair_load).  hi + lo carries 16 significant bits, so this is at most 2^-17 of a value;
  * `X3(drop_lo_hi=True)`, `X3(ninth_tap=True)`: two deliberately wrong emulations (a dropped cross term; the constant-input
    term of corner class 0 summing the tap above-left of the map as well) that test_dec_ref.py shows to be over the limit.

The limit of every compared tensor is `rule(emulation, ref64)` = max(4 x rel_err(emulation, ref64), 8 * 2^-24), relative to
max|ref64| and applied elementwise.  The factor 4 and the floor are the elementwise rule of glue_ref.f32_limit; here the factor
pays for what the emulation does not restate: the kernels' summation order (two accumulators, K slices over waves, the MFMA's
internal order) and `sigmoid_fast` (hardware exp2 and reciprocal, 1e-6 relative).  No limit depends on a kernel's output.

The weights are synthetic (`synth_sd`): every tensor decoder_fused.prep_gru / prep_flatten / prep_bev_update read, at the model's
shapes and at params.init_tensor's scale sqrt(2 / fan_in); biases and the BatchNorm weight, bias, mean and variance are distinct
per channel and away from 0 and 1, so a mis-indexed bias or scale is an error far above any limit.
"""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import glue_ref as G  # noqa: E402
from glue_ref import SENT, U32, Win, act_ref, check, check_equal, rel_err  # noqa: E402,F401

GRU_P = "gru"            # key prefixes of the synthetic state dict (prep_gru's `g`, prep_bev_update's `q`)
BEV_Q = "layer"
HW, PIX, C = 21, 441, 32
MIDS = 100 * 64 + 16 * 128 + 4 * 256
F64, F32 = torch.float64, torch.float32


# ----------------------------------------------------------------------------- the split and the three arithmetics
def split(x):
    """csrc/bf16x3.h: hi = rne_bf16(x), lo = rne_bf16(x - hi), both as f32 (torch's cast to bfloat16 rounds to nearest even)."""
    x = x.float()
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def pair_round(x):
    hi, lo = split(x)
    return hi + lo


class Plain:
    """Plain torch arithmetic in `dt`."""
    ninth_tap = False

    def __init__(self, dt):
        self.dt = dt

    def t(self, x):
        return x.to(self.dt)

    def conv(self, x, w, stride=1, pad=0):
        return F.conv2d(x, self.t(w), None, stride, pad)

    def lin(self, x, w):
        return x @ self.t(w).t()

    def hold(self, x):
        return x


class X3(Plain):
    """The bf16x3 emulation (module docstring)."""

    def __init__(self, drop_lo_hi=False, ninth_tap=False):
        super().__init__(F32)
        self.drop_lo_hi, self.ninth_tap = drop_lo_hi, ninth_tap

    def _three(self, op, x, w):
        xh, xl = split(x)
        wh, wl = split(w)
        y = op(xh, wh) + op(xh, wl)
        return y if self.drop_lo_hi else y + op(xl, wh)

    def conv(self, x, w, stride=1, pad=0):
        return self._three(lambda a, b: F.conv2d(a, b, None, stride, pad), x, w)

    def lin(self, x, w):
        return self._three(lambda a, b: a @ b.t(), x, w)

    def hold(self, x):
        return pair_round(x)


A64, A32 = Plain(F64), Plain(F32)


def rule(emu, ref64):
    """The limit of one compared tensor, relative to max|ref64|."""
    return max(4.0 * rel_err(emu, ref64), 8.0 * U32)


def check_rule(kernel, case, got, ref, limit, scale):
    """|got - ref| <= limit * scale elementwise, `scale` = max|ref64| of the WHOLE compared tensor (got / ref may be a part of
    it: one border class)."""
    check(kernel, case, got, ref, slack=limit * scale)


def _b(v):
    return v.view(1, -1, 1, 1)


# ----------------------------------------------------------------------------- border classes of a 3 x 3 / pad 1 conv
def border_classes():
    """[21, 21] long: 3 * row class + column class (0 first, 1 inside, 2 last), as border_class() of dec_spatial.hip."""
    k = torch.ones(HW, dtype=torch.long)
    k[0], k[-1] = 0, 2
    return 3 * k.view(HW, 1) + k.view(1, HW)


def valid_taps(ninth_tap=False):
    """[9, 21, 21]: tap (kh, kw) of the pixel lies inside the map.  `ninth_tap`: the wrong table, corner (0, 0) sums tap (0, 0) too."""
    y = torch.arange(HW)
    v = torch.zeros(9, HW, HW, dtype=torch.bool)
    for kh in range(3):
        for kw in range(3):
            oky, okx = (y + kh - 1 >= 0) & (y + kh - 1 < HW), (y + kw - 1 >= 0) & (y + kw - 1 < HW)
            v[kh * 3 + kw] = oky.view(HW, 1) & okx.view(1, HW)
    if ninth_tap:
        v[0, 0, 0] = True
    return v


def const_term(A, taps, bias):
    """The contribution of spatially constant input channels to a 3 x 3 / pad 1 conv: taps [B, 9, N] = W[n, const, tap] . x[b] ->
    [B, N, 21, 21], the sum over the taps inside the map (+ bias).  Plain arithmetic of A.dt (f32 in the kernels)."""
    return torch.einsum("btn,tyx->bnyx", taps, valid_taps(A.ninth_tap).to(A.dt)) + _b(A.t(bias))


# ----------------------------------------------------------------------------- SpatialGRU (dense_heads/utils.py:53-106)
def spatial_gru(A, sd, p, inp6, state, steps=4):
    """inp6 [B, 4, 6] (time-constant per step, spatially constant), state [B, 32, 21, 21] -> list of `steps` maps [B, 32, 21, 21].
    Every first conv reads cat([x, S]); its x part is the constant-input term."""
    def two(name, x6, s):
        W0 = sd[f"{p}.{name}.0.weight"]
        h = A.conv(s, W0[:, 6:], 1, 1)
        if x6 is None:
            h = h + _b(A.t(sd[f"{p}.{name}.0.bias"]))
        else:
            taps = torch.einsum("nckl,bc->bkln", A.t(W0[:, :6]), x6).reshape(x6.shape[0], 9, -1)
            h = h + const_term(A, taps, sd[f"{p}.{name}.0.bias"])
        return A.conv(torch.relu(h), sd[f"{p}.{name}.2.weight"], 1, 1) + _b(A.t(sd[f"{p}.{name}.2.bias"]))

    def decoder(s):
        h = torch.relu(A.conv(s, sd[f"{p}.conv_decoder.0.weight"], 1, 1) + _b(A.t(sd[f"{p}.conv_decoder.0.bias"])))
        return A.conv(h, sd[f"{p}.conv_decoder.2.weight"], 1, 1) + _b(A.t(sd[f"{p}.conv_decoder.2.bias"]))

    state = A.t(state)
    outs = []
    for t in range(steps):
        s = A.hold(state)
        x6 = A.t(inp6[:, t])
        u = torch.sigmoid(two("conv_update", x6, s))
        r = torch.sigmoid(two("conv_reset", x6, s))
        cand = two("conv_state_tilde", x6, (1.0 - r) * s)
        state = (1.0 - u) * s + u * cand
        outs.append(decoder(state))
    return outs


# ----------------------------------------------------------------------------- grid2feat (encoder_decoder_framework.py:228-234)
def _bn(A, sd, p, x, eps=1e-5):
    shape = (1, -1) + (1,) * (x.dim() - 2)
    w, b, m, v = (A.t(sd[f"{p}.{k}"]).view(shape) for k in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / torch.sqrt(v + eps) * w + b


def se_block(A, sd, p, x, lds):
    """SEBasicBlock (code/utils.py:84-121), pool = mean / 2 + max / 2.  `lds`: the level whose maps the kernel keeps in LDS."""
    hold = A.hold if lds else (lambda v: v)
    x = hold(x)
    y = torch.relu(_bn(A, sd, p + ".bn1", A.conv(x, sd[p + ".conv1.weight"], 1, 1) + _b(A.t(sd[p + ".conv1.bias"]))))
    y = hold(torch.relu(_bn(A, sd, p + ".bn2", A.conv(y, sd[p + ".conv2.weight"], 1, 1) + _b(A.t(sd[p + ".conv2.bias"])))))
    s = 0.5 * y.mean((2, 3), keepdim=True) + 0.5 * y.amax((2, 3), keepdim=True)
    s = torch.relu(A.conv(s, sd[p + ".se.fc1.weight"]) + _b(A.t(sd[p + ".se.fc1.bias"])))
    s = A.conv(s, sd[p + ".se.fc2.weight"]) + _b(A.t(sd[p + ".se.fc2.bias"]))
    return hold(torch.relu(y * torch.sigmoid(s) + x))


def grid2feat(A, sd, f21):
    """f21 [N, 32, 21, 21] -> (flat [N, 256], [f10 [N, 64, 10, 10], f4 [N, 128, 4, 4], f2 [N, 256, 2, 2]])."""
    def down(name, x, stride):
        return torch.relu(A.conv(x, sd[name + ".weight"], stride) + _b(A.t(sd[name + ".bias"])))
    f10 = se_block(A, sd, "MLP10", down("conv21_10", A.t(f21), 2), True)
    f4 = se_block(A, sd, "MLP4", down("conv10_4", f10, 2), False)
    f2 = se_block(A, sd, "MLP2", down("conv4_2", f4, 1), False)
    h = torch.relu(A.lin(f2.flatten(1), sd["output_fc.0.weight"]) + A.t(sd["output_fc.0.bias"]))
    h = _bn(A, sd, "output_fc.2", h)
    return torch.relu(A.lin(h, sd["output_fc.3.weight"]) + A.t(sd["output_fc.3.bias"])), [f10, f4, f2]


def mids_of(mids):
    """The kernel's `mids` rows [N, 9472] (pixel-major, channel-minor per level) -> the three maps, channel first."""
    n = mids.shape[0]
    return [mids[:, :6400].reshape(n, 10, 10, 64).permute(0, 3, 1, 2), mids[:, 6400:8448].reshape(n, 4, 4, 128).permute(0, 3, 1, 2),
            mids[:, 8448:].reshape(n, 2, 2, 256).permute(0, 3, 1, 2)]


# ----------------------------------------------------------------------------- BEV update (thinktwice_decoder.py:221-225,257)
def bev_g(A, sd, q, hb):
    """The broadcast-channel term G[b, tap * 128 + n] = W0[n, 32:, tap] . hb[b]  (one linear over the B rows: a row chain)."""
    W0 = sd[q + ".BEV_feat_update_module.0.weight"]
    return A.lin(A.t(hb), W0[:, 32:].permute(2, 3, 0, 1).reshape(9 * 128, -1))


def bev_update(A, sd, q, bev, hb, g=None):
    """conv2(relu(conv0(cat[bev, hb broadcast]))) + bev: bev [B, 32, 21, 21], hb [B, 2048] -> [B, 32, 21, 21]."""
    m = q + ".BEV_feat_update_module"
    g = bev_g(A, sd, q, hb) if g is None else A.t(g)
    bev = A.t(bev)
    h = A.conv(bev, sd[m + ".0.weight"][:, :32], 1, 1) + const_term(A, g.reshape(-1, 9, 128), sd[m + ".0.bias"])
    return A.conv(torch.relu(h), sd[m + ".2.weight"], 1, 1) + _b(A.t(sd[m + ".2.bias"])) + bev


# ----------------------------------------------------------------------------- a row chain (include/thinktwice_hip.h: tt_chain_stage)
def chain(A, x, stages):
    """stage: dict(w [N, side_k + K], bias [N] | None, act, src (-1: x[:, :K]), side_k, side [R, >= side_k] | None,
    res [R, >= res_coff + N] | None, res_coff) -> the list of every stage's output [R, N]:
    act(W . in + bias + side_w . side + res)."""
    outs = []
    for st in stages:
        sk = st.get("side_k", 0)
        w = st["w"]
        K = w.shape[1] - sk
        inp = A.t(x[:, :K]) if st["src"] < 0 else outs[st["src"]]
        v = A.lin(inp, w[:, sk:])
        if st.get("bias") is not None:
            v = v + A.t(st["bias"])
        if sk:
            v = v + A.t(st["side"][:, :sk]) @ A.t(w[:, :sk]).t()
        if st.get("res") is not None:
            v = v + A.t(st["res"][:, st["res_coff"]:st["res_coff"] + w.shape[0]])
        outs.append(act_ref(v, st.get("act", 0)))
    return outs


# ----------------------------------------------------------------------------- the synthetic state dict
def synth_sd(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def away(n, lo, hi, signed=True):          # distinct per channel, |v| in [lo, hi): away from 0 (and, by the range, from 1)
        v = lo + (hi - lo) * torch.rand(n, generator=g)
        return v * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float() if signed else v

    def conv(name, cout, cin, k):
        sd[name + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        sd[name + ".bias"] = away(cout, 0.03, 0.15)

    def lin(name, cout, cin):
        sd[name + ".weight"] = torch.randn(cout, cin, generator=g) * (2.0 / cin) ** 0.5
        sd[name + ".bias"] = away(cout, 0.03, 0.15)

    def bn(name, c):
        sd[name + ".weight"] = away(c, 0.55, 0.9, signed=False)
        sd[name + ".bias"] = away(c, 0.05, 0.25)
        sd[name + ".running_mean"] = away(c, 0.05, 0.25)
        sd[name + ".running_var"] = away(c, 0.4, 0.9, signed=False)

    for n in ("conv_update", "conv_reset", "conv_state_tilde"):
        conv(f"{GRU_P}.{n}.0", 32, 38, 3)
        conv(f"{GRU_P}.{n}.2", 32, 32, 3)
    conv(f"{GRU_P}.conv_decoder.0", 32, 32, 3)
    conv(f"{GRU_P}.conv_decoder.2", 32, 32, 3)
    conv("conv21_10", 64, 32, 3)
    conv("conv10_4", 128, 64, 3)
    conv("conv4_2", 256, 128, 3)
    for name, c in (("MLP10", 64), ("MLP4", 128), ("MLP2", 256)):
        conv(name + ".conv1", 2 * c, c, 3)
        bn(name + ".bn1", 2 * c)
        conv(name + ".conv2", c, 2 * c, 3)
        bn(name + ".bn2", c)
        conv(name + ".se.fc1", c, c, 1)
        conv(name + ".se.fc2", c, c, 1)
    lin("output_fc.0", 512, 1024)
    bn("output_fc.2", 512)
    lin("output_fc.3", 256, 512)
    conv(BEV_Q + ".BEV_feat_update_module.0", 128, 2080, 3)
    conv(BEV_Q + ".BEV_feat_update_module.2", 32, 128, 3)
    return sd


@functools.lru_cache(None)
def sd_std():
    return synth_sd(0)


@functools.lru_cache(None)
def sd_saturated():
    """Gates driven into saturation: +-12 (sigmoid within 1e-5 of 0 / 1) and +-100 (exp2 overflow / flush of sigmoid_fast)."""
    sd = dict(sd_std())
    for n in ("conv_update", "conv_reset"):
        b = sd[f"{GRU_P}.{n}.2.bias"].clone()
        b[0:8] += 12.0
        b[8:16] -= 12.0
        b[16:18] += 100.0
        b[18:20] -= 100.0
        sd[f"{GRU_P}.{n}.2.bias"] = b
    return sd


# ----------------------------------------------------------------------------- cases (inputs, float64 reference, limits): computed once
def _evals(fn):
    """fn(A) -> list of tensors; -> dict(ref, emu, f32, limit, scale) with one entry per tensor."""
    with torch.no_grad():
        ref, emu, f32 = fn(A64), fn(X3()), fn(A32)
    return {"ref": ref, "emu": emu, "f32": f32, "limit": [rule(e, r) for e, r in zip(emu, ref)],
            "scale": [float(r.abs().max()) for r in ref]}


GRU_CASES = ("B1", "B2", "B5", "saturated", "zero", "big-input")


@functools.lru_cache(None)
def gru_case(name):
    """dict(sd, B, inp6 [B, 4, 6], state [B, 32, 21, 21], ref / emu / f32: 4 maps each, limit / scale: per step)."""
    g = torch.Generator().manual_seed(21)
    inp6 = torch.randn(5, 4, 6, generator=g)
    state = torch.randn(5, 32, HW, HW, generator=g) * 0.5
    sd = sd_std()
    if name in ("B1", "B2", "B5"):
        B = int(name[1:])
    elif name == "saturated":
        B, sd = 2, sd_saturated()
    elif name == "zero":                                    # bias and constant-term path only
        B, inp6, state = 1, torch.zeros_like(inp6), torch.zeros_like(state)
    elif name == "big-input":
        # the constant-input term dominates: the largest input is 10.  (Every input at +-10 drives the step-3 and step-4 maps
        # to 20 and the emulation's own error to 2.7e-5: that limit, 1.1e-4, is outside the window test_dec_ref.py asserts.)
        B = 1
        inp6 = inp6 * (10.0 / float(inp6[:1].abs().max()))
        state = state * 0.1
    else:
        raise KeyError(name)
    inp6, state = inp6[:B].contiguous(), state[:B].contiguous()
    c = _evals(lambda A: spatial_gru(A, sd, GRU_P, inp6, state))
    c.update(sd=sd, B=B, inp6=inp6, state=state)
    return c


FLAT_MAPS = (1, 4, 5, 17, 32, 33)
FLAT_CASES = tuple(f"maps{n}" for n in FLAT_MAPS) + ("all-negative", "corner-maximum")


@functools.lru_cache(None)
def _flat_pool():
    """33 signed maps, an all-negative one and one whose maximum sits in corner pixel (20, 20) of channel 5, with every evaluation
    (grid2feat treats the maps independently: eval BatchNorm)."""
    g = torch.Generator().manual_seed(5)
    f21 = torch.randn(35, 32, HW, HW, generator=g) * 0.7
    f21[33] = -f21[33].abs()
    f21[34, 5, 20, 20] = 6.0
    sd = sd_std()

    def run(A):
        flat, mids = grid2feat(A, sd, f21)
        return mids + [flat]
    with torch.no_grad():
        return f21, run(A64), run(X3()), run(A32)


FLAT_OUT = ("f10", "f4", "f2", "flat")


@functools.lru_cache(None)
def flat_case(name):
    """dict(sd, maps [n, 32, 21, 21], ref / emu / f32 / limit / scale per tensor of FLAT_OUT).  The edge cases are launches of three
    maps with the special one in the middle."""
    f21, ref, emu, f32 = _flat_pool()
    idx = {"all-negative": [0, 33, 1], "corner-maximum": [0, 34, 1]}.get(name) or list(range(int(name[4:])))
    ref, emu, f32 = ([t[idx] for t in ts] for ts in (ref, emu, f32))
    return {"sd": sd_std(), "maps": f21[idx].contiguous(), "ref": ref, "emu": emu, "f32": f32,
            "limit": [rule(e, r) for e, r in zip(emu, ref)], "scale": [float(r.abs().max()) for r in ref]}


BEV_CASES = ("B1", "B3")


@functools.lru_cache(None)
def bev_case(name):
    """dict(sd, B, bev [B, 32, 21, 21], hb [B, 2048], ref / emu / f32 / limit / scale for [G [B, 1152], out [B, 32, 21, 21]])."""
    B = int(name[1:])
    g = torch.Generator().manual_seed(11)
    bev = (torch.randn(3, 32, HW, HW, generator=g) * 0.5)[:B].contiguous()
    hb = (torch.randn(3, 2048, generator=g).abs() * 0.3)[:B].contiguous()
    sd = sd_std()
    c = _evals(lambda A: [bev_g(A, sd, BEV_Q, hb), bev_update(A, sd, BEV_Q, bev, hb)])
    c.update(sd=sd, B=B, bev=bev, hb=hb)
    return c


# ---- row chains.  x rows carry SENT from column K on (row stride Kp + 4): the header promises the kernels only "finite padding"
def _lin(g, n, k):
    return torch.randn(n, k, generator=g) * k ** -0.5, torch.randn(n, generator=g) * 0.1


def _rows(g, R, K):
    Kp = (K + 15) // 16 * 16
    x = torch.full((R, Kp + 4), SENT)
    x[:, :K] = torch.randn(R, K, generator=g)
    return x


SINGLE = ((1, 16, 2), (31, 32, 31), (33, 48, 33), (64, 80, 100), (65, 272, 288), (96, 528, 32), (129, 20, 4))
CHAIN_CASES = (tuple(f"single-R{r}-K{k}-N{n}" for r, k, n in SINGLE) + ("ragged-middle-R33", "ragged-middle-R65") +
               tuple(f"res-side{sk}-R{r}" for sk in (2, 8) for r in (45, 129)) +
               tuple("act-" + G.ACT_NAMES[a] for a in range(6)) + ("split-N96",))


@functools.lru_cache(None)
def chain_case(name):
    """dict(R, x, stages (dec_ref.chain's dicts; "out": True where the stage's output is written and compared), ref / emu / f32 /
    limit / scale: one entry per stage with "out")."""
    g = torch.Generator().manual_seed(sum(name.encode()))
    part = name.split("-")
    if part[0] == "single":
        R, K, N = (int(p[1:]) for p in part[1:])
        w, b = _lin(g, N, K)
        stages = [dict(w=w, bias=b, act=0, src=-1, out=True)]
    elif part[0] == "ragged":                     # 64 -> 100 (ReLU) -> 8: stage 2 has K = 100, Kp = 112 and reads zero padding
        R, K = int(part[2][1:]), 64
        w1, b1 = _lin(g, 100, 64)
        w2, b2 = _lin(g, 8, 100)
        stages = [dict(w=w1, bias=b1, act=G.ACT_RELU, src=-1), dict(w=w2, bias=b2, act=0, src=0, out=True)]
    elif part[0] == "res":                        # residual at res_stride N + 12, res_coff 8; side input at side_stride 12
        sk, R, K, N = int(part[1][4:]), int(part[2][1:]), 64, 40
        w, b = _lin(g, N, sk + K)
        stages = [dict(w=w, bias=b, act=G.ACT_RELU, src=-1, side_k=sk, side=torch.randn(R, 12, generator=g),
                       res=torch.randn(R, N + 12, generator=g), res_coff=8, out=True)]
    elif part[0] == "act":
        R, K, N = 37, 64, 40
        w, b = _lin(g, N, K)
        w = w * 2.0                               # pre-activations of a few units: both tails of every activation
        stages = [dict(w=w, bias=b, act={v: k for k, v in G.ACT_NAMES.items()}[part[1]], src=-1, out=True)]
    elif part[0] == "split":                      # N = 96: three column blocks
        R, K, N = 40, 64, 96
        w, b = _lin(g, N, K)
        stages = [dict(w=w, bias=b, act=0, src=-1, out=True)]
    else:
        raise KeyError(name)
    x = _rows(g, R, K)
    keep = [i for i, s in enumerate(stages) if s.get("out")]
    c = _evals(lambda A: [chain(A, x, stages)[i] for i in keep])
    c.update(R=R, x=x, stages=stages)
    return c
