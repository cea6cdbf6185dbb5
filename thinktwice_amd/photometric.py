"""Colour augmentation of training frames on the device: ImageTransformMulti(aug=True) and its imgaug `augmenter(iteration)`
(open_loop_training/code/datasets/pipelines/transform.py:142-216).  The host side: the schedule of the nine factors, the
sampler of one *program* per sample, and the compiler of a draw into the device steps of tt_aug_program
(include/thinktwice_hip.h); the kernels (csrc/photometric.hip) only execute tables.

What matches the reference: the schedule, the operator set, the laws of the draws, the sharing rule (one order, one set of
parameters and one per-pixel random field for all T x N frames of a sample: `to_deterministic()`) and the uint8 arithmetic.
What does not: imgaug's random stream is not reproduced draw for draw.

[3P] unpinned.  imgaug and cv2 were not installed where this was written, so no fixture pins their arithmetic.  Every
rounding convention taken from imgaug 0.4.0 / cv2 semantics lives in ONE host function each -- `add_lut`, `multiply_lut`,
`contrast_lut`, `noise_thresholds`, `dropout_threshold`, `coarse_grid`, `gray_alpha` (with the device's fixed BT.601 weights),
`blur_taps` -- so that a session that has imgaug can pin them by editing those functions and nothing else.

Order of the draws of one sample on the RandomState (PhotometricSampler.sample_one):
  1. `permutation(8)`: the execution order of OPERATORS;
  2. then, for each operator IN EXECUTION ORDER: `uniform()` (applied when < frequency), and only when applied
       blur      sigma = uniform(0, blur)
       noise     uniform() (per-channel when < color), scale = uniform(0, dropout), seed
       coarse    uniform() (per-channel), p = uniform(0, dropout), ph = uniform(0.08, 0.2), pw = uniform(0.08, 0.2), seed
       dropout   uniform() (per-channel), p = uniform(0, dropout), seed
       add       uniform() (per-channel), then 3 (per-channel) or 1 x uniform(-add, add)
       multiply  uniform() (per-channel), then 3 or 1 x uniform(mul_neg, mul_pos)
       contrast  uniform() (per-channel), then 3 or 1 x uniform(con_neg, con_pos)
       gray      alpha = uniform(0, 1)
     where seed = (randint(0, 2**32) << 32) | randint(0, 2**32), two draws of dtype uint64."""
import collections
import ctypes
import math

import numpy as np

from . import _lib, ops
from ._lib import (TT_AUG_BLUR as BLUR, TT_AUG_COARSE as COARSE, TT_AUG_DROPOUT as DROPOUT, TT_AUG_GRAY as GRAY,  # noqa: F401
                   TT_AUG_LUT as LUT, TT_AUG_MAX_OPS, TT_AUG_NOISE as NOISE, TT_AUG_NOISE_K)
from .ops import check, lib, ptr

KIND_NAMES = ("LUT", "NOISE", "DROPOUT", "COARSE", "GRAY", "BLUR")
OPERATORS = ("blur", "noise", "coarse", "dropout", "add", "multiply", "contrast", "gray")      # augmenter()'s list order
MAX_NOISE_SCALE = 0.5        # the mass of N(0, 0.5) beyond +-4.5 is 2.3e-19; the schedule never exceeds 0.199


AugOp, AugProgram = _lib.structs()["tt_aug_op"], _lib.structs()["tt_aug_program"]


class PhotometricSchedule:
    """The nine factors of augmenter(iteration) (transform.py:171-185), in Python floats exactly as written there."""

    def __init__(self, iteration):
        it = self.iteration = iteration
        self.frequency = min(0.05 + float(it) / 600000.0, 1.0)
        self.color = min(float(it) / 3000000.0, 1.0)
        self.dropout = 0.198667 + (0.03856658 - 0.198667) / (1 + (it / 600000) ** 1.863486)
        self.blur = min(0.5 + (0.5 * it / 300000.0), 1.0)
        self.add = 10 + 10 * it / 300000.0
        self.mul_pos = 1 + (2.5 * it / 600000.0)
        self.mul_neg = 1 - (0.91 * it / 1500000.0)
        self.con_pos = 1 + (0.5 * it / 1500000.0)
        self.con_neg = 1 - (0.5 * it / 1500000.0)


# one applied operator of a draw: `values` are its parameters in the docstring's order (per channel: three of them)
OpDraw = collections.namedtuple("OpDraw", "name per_channel values seed")
# one sample's draw: the execution order of all eight operators and the applied ones, in that order
PhotometricDraw = collections.namedtuple("PhotometricDraw", "iteration order ops")


class PhotometricSampler:
    """One draw per sample on a numpy RandomState (a seed or an instance, like IdaSampler).  Sample number `reads` is drawn
    at iteration reads / batch_size, then reads += 1: ImageTransformMulti's `_batch_read_number / _batch_size`."""

    def __init__(self, batch_size, seed=None, reads=0):
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        self.batch_size = batch_size
        self.reads = reads
        self.rng = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)

    def _seed(self):
        hi = int(self.rng.randint(0, 2 ** 32, dtype=np.uint64))
        return (hi << 32) | int(self.rng.randint(0, 2 ** 32, dtype=np.uint64))

    def sample_one(self, iteration):
        s, rng = PhotometricSchedule(iteration), self.rng
        order = tuple(OPERATORS[i] for i in rng.permutation(len(OPERATORS)))
        ops = []
        for name in order:
            if not rng.uniform() < s.frequency:
                continue
            if name == "blur":
                ops.append(OpDraw(name, False, (rng.uniform(0, s.blur),), None))
            elif name == "gray":
                ops.append(OpDraw(name, False, (rng.uniform(0, 1),), None))
            else:
                pc = bool(rng.uniform() < s.color)
                if name == "noise":
                    ops.append(OpDraw(name, pc, (rng.uniform(0, s.dropout),), self._seed()))
                elif name == "coarse":
                    v = (rng.uniform(0, s.dropout), rng.uniform(0.08, 0.2), rng.uniform(0.08, 0.2))
                    ops.append(OpDraw(name, pc, v, self._seed()))
                elif name == "dropout":
                    ops.append(OpDraw(name, pc, (rng.uniform(0, s.dropout),), self._seed()))
                else:
                    lo, hi = {"add": (-s.add, s.add), "multiply": (s.mul_neg, s.mul_pos), "contrast": (s.con_neg, s.con_pos)}[name]
                    ops.append(OpDraw(name, pc, tuple(rng.uniform(lo, hi) for _ in range(3 if pc else 1)), None))
        return PhotometricDraw(iteration, order, tuple(ops))

    def sample(self, B, iteration=None):
        """B draws.  `iteration` overrides the read counter (which then stands still)."""
        out = []
        for _ in range(B):
            if iteration is None:
                out.append(self.sample_one(self.reads / self.batch_size))
                self.reads += 1
            else:
                out.append(self.sample_one(iteration))
        return out

    def programs(self, B, H, W, iteration=None):
        return [compile_program(d, H, W) for d in self.sample(B, iteration)]


# ------------------------------------------------------------------------------------ the adopted conventions, one function each
def _clip_u8(a):
    return np.clip(a, 0, 255).astype(np.uint8)


def add_lut(value):
    """iaa.Add on uint8: the value is rounded to an integer (ties to even) and added with saturation."""
    k = int(np.rint(value))
    return _clip_u8(np.arange(256, dtype=np.int64) + k)


def multiply_lut(m):
    """iaa.Multiply on uint8: f32 product, rounded (ties to even), saturated."""
    return _clip_u8(np.rint(np.arange(256, dtype=np.float32) * np.float32(m)))


def contrast_lut(alpha):
    """iaa.LinearContrast on uint8: 127 + alpha * (v - 127) in f32, rounded (ties to even), saturated."""
    i = np.arange(256, dtype=np.float32)
    return _clip_u8(np.rint(np.float32(127) + np.float32(alpha) * (i - np.float32(127))))


def _phi(z):
    return 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))


def noise_thresholds(scale):
    """iaa.AdditiveGaussianNoise on uint8 adds round(N(0, scale)) with saturation.  The law of k = round(N(0, scale)) on
    -K..K as cumulative u32 thresholds: cum[j] = floor(2^32 * Phi((-K + j + 0.5) / scale)), computed in f64; for a 32-bit
    field value u, k = -K + #{j : u >= cum[j]}.  A cum of 2^32 (never reached) saturates to 2^32 - 1."""
    if not 0 < scale <= MAX_NOISE_SCALE:
        raise ValueError(f"noise scale {scale} outside (0, {MAX_NOISE_SCALE}]")
    K = TT_AUG_NOISE_K
    cum = []
    for j in range(2 * K):
        cum.append(min(int(math.floor(2.0 ** 32 * _phi((-K + j + 0.5) / scale))), 2 ** 32 - 1))
    return tuple(cum)


def noise_is_zero(scale):
    """Whether round(N(0, scale)) is 0 for every 32-bit field value: no mass below -0.5, all of it below 0.5."""
    return scale <= 0 or (math.floor(2.0 ** 32 * _phi(-0.5 / scale)) == 0 and math.floor(2.0 ** 32 * _phi(0.5 / scale)) == 2 ** 32)


def dropout_threshold(p):
    """iaa.Dropout / CoarseDropout: an element is zeroed with probability p: u < floor(p * 2^32)."""
    if not 0 <= p <= 1:
        raise ValueError(f"dropout probability {p} outside [0, 1]")
    return min(int(math.floor(p * 2.0 ** 32)), 2 ** 32 - 1)


def coarse_grid(H, W, ph, pw):
    """iaa.CoarseDropout(size_percent): the mask is drawn on a (max(int(H * ph), 3), max(int(W * pw), 3)) grid and enlarged
    to the image with nearest-neighbour cells: pixel (y, x) lies in cell (y * gh // H, x * gw // W)."""
    return max(int(H * ph), 3), max(int(W * pw), 3)


def gray_alpha(alpha):
    """iaa.Grayscale(alpha): out = v + alpha * (gray - v) in f32, gray the fixed-point BT.601 luma cv2 uses for uint8
    ((4899 R + 9617 G + 1868 B + 8192) >> 14, on the device)."""
    if not 0 <= alpha <= 1:
        raise ValueError(f"grayscale alpha {alpha} outside [0, 1]")
    return float(np.float32(alpha))


def blur_taps(sigma):
    """iaa.GaussianBlur through cv2.GaussianBlur: kernel size max(3.3 * sigma, 5) -> 5 for every sigma <= 1, taps
    exp(-i^2 / (2 sigma^2)) normalised in f64, then f32; border reflect-101."""
    if not 1e-3 <= sigma <= 1.0:
        raise ValueError(f"blur sigma {sigma} outside [1e-3, 1] (a 5-tap kernel)")
    g = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(-2, 3)]
    t = sum(g)
    return tuple(float(np.float32(x / t)) for x in g)


# ------------------------------------------------------------------------------------------------------ programs
# one device step (the fields a kind does not use are None)
Step = collections.namedtuple("Step", "kind per_channel grid threshold alpha seed cum taps lut", defaults=(None,) * 8)


class Program:
    """A sample's compiled program: the ordered device steps, for images of H x W."""

    def __init__(self, steps=(), H=None, W=None):
        self.steps, self.H, self.W = list(steps), H, W

    def __len__(self):
        return len(self.steps)

    def __eq__(self, other):
        return isinstance(other, Program) and (self.H, self.W) == (other.H, other.W) and len(self) == len(other) and all(
            _step_key(a) == _step_key(b) for a, b in zip(self.steps, other.steps))

    def __repr__(self):
        return f"Program({[KIND_NAMES[s.kind] if 0 <= s.kind < len(KIND_NAMES) else s.kind for s in self.steps]}, {self.H} x {self.W})"

    @property
    def blur_index(self):
        return next((i for i, s in enumerate(self.steps) if s.kind == BLUR), -1)

    def pack(self):
        p = AugProgram()
        p.num_ops, p.blur_index = len(self.steps), self.blur_index
        for o, s in zip(p.ops, self.steps):
            o.kind, o.per_channel = s.kind, int(bool(s.per_channel))
            if s.grid is not None:
                o.grid_h, o.grid_w = s.grid
            if s.threshold is not None:
                o.threshold = s.threshold
            if s.alpha is not None:
                o.alpha = s.alpha
            if s.seed is not None:
                o.seed = s.seed
            if s.cum is not None:
                o.cum[:] = s.cum
            if s.taps is not None:
                o.taps[:] = s.taps
            if s.lut is not None:
                ctypes.memmove(o.lut, np.ascontiguousarray(s.lut, dtype=np.uint8).ctypes.data, 768)
        return p


def _step_key(s):
    return tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in s)


def compile_program(draw, H, W):
    """The ordered device steps of a draw for H x W images.  Add / Multiply / LinearContrast become LUT steps, adjacent LUT
    steps are composed (exact: uint8 -> uint8 maps); a blur of sigma < 1e-3 is dropped (imgaug's rule), and so is a noise
    whose rounded value is 0 with certainty."""
    steps = []
    for op in draw.ops:
        v = op.values
        if op.name in ("add", "multiply", "contrast"):
            f = {"add": add_lut, "multiply": multiply_lut, "contrast": contrast_lut}[op.name]
            lut = np.stack([f(v[c if op.per_channel else 0]) for c in range(3)])
            if steps and steps[-1].kind == LUT:
                lut = np.stack([lut[c][steps[-1].lut[c]] for c in range(3)])
                steps.pop()
            steps.append(Step(LUT, lut=lut))
        elif op.name == "noise":
            if noise_is_zero(v[0]):
                continue
            steps.append(Step(NOISE, op.per_channel, seed=op.seed, cum=noise_thresholds(v[0])))
        elif op.name == "dropout":
            steps.append(Step(DROPOUT, op.per_channel, threshold=dropout_threshold(v[0]), seed=op.seed))
        elif op.name == "coarse":
            steps.append(Step(COARSE, op.per_channel, grid=coarse_grid(H, W, v[1], v[2]), threshold=dropout_threshold(v[0]),
                              seed=op.seed))
        elif op.name == "gray":
            steps.append(Step(GRAY, alpha=gray_alpha(v[0])))
        elif op.name == "blur":
            if v[0] < 1e-3:
                continue
            steps.append(Step(BLUR, taps=blur_taps(v[0])))
        else:
            raise ValueError(f"unknown operator {op.name!r}")
    prog = Program(steps, H, W)
    check_programs([prog], 1, H, W)
    return prog


def check_programs(programs, B, H, W):
    """ValueError, naming the sample, for programs the device entries would refuse (their host check, restated)."""
    if len(programs) != B or not all(isinstance(p, Program) for p in programs):
        raise ValueError(f"need {B} compiled programs (photometric.Program)")
    for b, p in enumerate(programs):
        if len(p) > TT_AUG_MAX_OPS:
            raise ValueError(f"sample {b}: {len(p)} steps, at most {TT_AUG_MAX_OPS}")
        if (p.H, p.W) not in ((H, W), (None, None)):
            raise ValueError(f"sample {b}: compiled for {p.H} x {p.W} images, the call has {H} x {W}")
        if sum(s.kind == BLUR for s in p.steps) > 1:
            raise ValueError(f"sample {b}: more than one blur")
        for k, s in enumerate(p.steps):
            where = f"sample {b} step {k}"
            if s.kind == LUT:
                if s.lut is None or np.asarray(s.lut).shape != (3, 256) or np.asarray(s.lut).dtype != np.uint8:
                    raise ValueError(f"{where}: a LUT step needs a uint8 [3, 256] table")
            elif s.kind == NOISE:
                c = s.cum
                if c is None or len(c) != 2 * TT_AUG_NOISE_K or any(not 0 <= x < 2 ** 32 for x in c) or list(c) != sorted(c):
                    raise ValueError(f"{where}: noise thresholds must be {2 * TT_AUG_NOISE_K} non-decreasing u32")
            elif s.kind in (DROPOUT, COARSE):
                if s.threshold is None or not 0 <= s.threshold < 2 ** 32:
                    raise ValueError(f"{where}: threshold must be a u32")
                if s.kind == COARSE and (s.grid is None or not (1 <= s.grid[0] <= H and 1 <= s.grid[1] <= W)):
                    raise ValueError(f"{where}: grid {s.grid} outside 1..{H} x 1..{W}")
            elif s.kind == GRAY:
                if s.alpha is None or not 0 <= s.alpha <= 1:
                    raise ValueError(f"{where}: alpha {s.alpha} outside [0, 1]")
            elif s.kind == BLUR:
                t = s.taps
                if t is None or len(t) != 5 or not all(math.isfinite(x) and x >= 0 for x in t) or abs(sum(t) - 1) > 1e-5:
                    raise ValueError(f"{where}: blur taps {t} must be five finite non-negative values summing to 1")
                if H < 3 or W < 3:
                    raise ValueError(f"{where}: a blur needs H, W >= 3, got {H} x {W}")
            else:
                raise ValueError(f"{where}: unknown kind {s.kind}")
            if s.kind in (NOISE, DROPOUT, COARSE) and (s.seed is None or not 0 <= s.seed < 2 ** 64):
                raise ValueError(f"{where}: the field seed must be a u64")


def pack_programs(programs):
    """The B programs as one CPU uint8 tensor [B, sizeof(tt_aug_program)] (the entries' host copy; `.to(device)` of it is
    their device copy)."""
    import torch
    arr = (AugProgram * len(programs))(*[p.pack() for p in programs])
    return torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).reshape(len(programs), ctypes.sizeof(AugProgram)).copy())


def scratch_bytes(num_images, H, W):
    """tt_photometric_scratch_bytes: one packed 4-byte pixel per pixel."""
    return num_images * H * W * 4


def device_programs(programs, num_images, H, W, device, pinned=False):
    """(host tensor, device tensor, scratch tensor or None, scratch bytes) of a call over `num_images` images: the scratch
    comes from torch's caching allocator, and only when a program has a blur.  pinned: the host copy is page-locked and goes
    up without the host waiting for the stream (loader.py queues it behind a decode it must not wait for); the default, a
    pageable copy, synchronises the current stream."""
    import torch
    host = pack_programs(programs)
    if pinned:
        host = host.pin_memory()
    dev = host.to(device, non_blocking=pinned)
    scratch, nbytes = None, 0
    if any(p.blur_index >= 0 for p in programs):
        nbytes = scratch_bytes(num_images, H, W)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return host, dev, scratch, nbytes


def apply_u8(images_u8, programs):
    """uint8 [B, K, H, W, 3] on the device under B compiled programs (image (b, k) under program b) -> uint8 of that shape."""
    import torch
    if images_u8.dim() != 5 or images_u8.dtype != torch.uint8 or images_u8.shape[-1] != 3 or not images_u8.is_contiguous():
        raise ValueError("images must be a contiguous uint8 [B, K, H, W, 3] tensor")
    B, K, H, W, _ = images_u8.shape
    if B == 0 or K == 0:
        raise ValueError("images must be a non-empty [B, K, H, W, 3] tensor")
    check_programs(programs, B, H, W)                   # (nothing has been launched before this line)
    _lib.require_cuda(images_u8)
    host, dev, scratch, nbytes = device_programs(programs, B * K, H, W, images_u8.device)
    out = torch.empty_like(images_u8)
    check(lib().tt_photometric_u8(ptr(images_u8), B, K, H, W, host.data_ptr(), ptr(dev), ptr(scratch), nbytes, ptr(out),
                                  ops.cur_stream(images_u8.device)), "tt_photometric_u8")
    return out
