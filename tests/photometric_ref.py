"""numpy restatement of the device's photometric stage (csrc/photometric.hip; the step arithmetic is stated in
include/thinktwice_hip.h at tt_aug_op): `field` is the per-element random field, `apply_program` runs a compiled
thinktwice_amd.photometric.Program on one uint8 image.  uint64 and f32 arithmetic in the device's operation order, so the
device is expected to agree with it in every byte."""
import numpy as np

from thinktwice_amd import photometric as P

_GOLD = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def field(seed, n):
    """u32 field values of elements 0..n-1: the high 32 bits of the splitmix64 mix at seed + GOLD * (idx + 1)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + _GOLD * (np.arange(n, dtype=np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def field_image(seed, per_channel, h, w):
    """[h, w, 3] field: idx = (c * h + y) * w + x per channel, else y * w + x shared by the channels."""
    if per_channel:
        return np.ascontiguousarray(field(seed, 3 * h * w).reshape(3, h, w).transpose(1, 2, 0))
    return np.repeat(field(seed, h * w).reshape(h, w, 1), 3, axis=2)


def noise_k(u, cum):
    """k = -K + #{j : u >= cum[j]}"""
    k = np.full(u.shape, -P.TT_AUG_NOISE_K, dtype=np.int64)
    for c in cum:
        k += u >= np.uint32(c)
    return k


def coarse_mask(step, H, W):
    """[H, W, 3] bool: the dropped elements of a COARSE step."""
    gh, gw = step.grid
    u = field_image(step.seed, step.per_channel, gh, gw)
    cy = np.arange(H, dtype=np.int64) * gh // H
    cx = np.arange(W, dtype=np.int64) * gw // W
    return u[cy[:, None], cx[None, :]] < np.uint32(step.threshold)


def _reflect101(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def blur(img, taps):
    """5 x 5 separable blur of an int [H, W, 3] image, reflect-101: horizontal then vertical in f32, each summed
    ((((g0 p0 + g1 p1) + g2 p2) + g3 p3) + g4 p4); rint (ties to even), clip."""
    H, W, _ = img.shape
    g = [np.float32(t) for t in taps]
    f = img.astype(np.float32)
    xs = [_reflect101(np.arange(W) + k - 2, W) for k in range(5)]
    ys = [_reflect101(np.arange(H) + k - 2, H) for k in range(5)]
    h = g[0] * f[:, xs[0]] + g[1] * f[:, xs[1]]
    for k in range(2, 5):
        h = h + g[k] * f[:, xs[k]]
    v = g[0] * h[ys[0]] + g[1] * h[ys[1]]
    for k in range(2, 5):
        v = v + g[k] * h[ys[k]]
    assert h.dtype == v.dtype == np.float32
    return np.clip(np.rint(v), 0, 255).astype(np.int64)


def apply_step(v, s):
    """One step on an int64 [H, W, 3] image of grey levels."""
    H, W, _ = v.shape
    if s.kind == P.LUT:
        lut = np.asarray(s.lut)
        return np.stack([lut[c][v[..., c]] for c in range(3)], axis=-1).astype(np.int64)
    if s.kind == P.NOISE:
        return np.clip(v + noise_k(field_image(s.seed, s.per_channel, H, W), s.cum), 0, 255)
    if s.kind == P.DROPOUT:
        return np.where(field_image(s.seed, s.per_channel, H, W) < np.uint32(s.threshold), 0, v)
    if s.kind == P.COARSE:
        return np.where(coarse_mask(s, H, W), 0, v)
    if s.kind == P.GRAY:
        g = (4899 * v[..., 0] + 9617 * v[..., 1] + 1868 * v[..., 2] + 8192) >> 14
        f = v.astype(np.float32) + np.float32(s.alpha) * (g[..., None] - v).astype(np.float32)
        assert f.dtype == np.float32
        return np.clip(np.rint(f), 0, 255).astype(np.int64)
    if s.kind == P.BLUR:
        return blur(v, s.taps)
    raise ValueError(f"unknown step kind {s.kind}")


def apply_program(image_u8, program):
    """uint8 [H, W, 3] -> uint8 [H, W, 3] under a compiled program."""
    v = np.asarray(image_u8).astype(np.int64)
    for s in program.steps:
        v = apply_step(v, s)
    return v.astype(np.uint8)


def apply_batch(images_u8, programs):
    """uint8 [B, K, H, W, 3] under B programs, as photometric.apply_u8."""
    out = np.empty_like(images_u8)
    for b, p in enumerate(programs):
        for k in range(images_u8.shape[1]):
            out[b, k] = apply_program(images_u8[b, k], p)
    return out
