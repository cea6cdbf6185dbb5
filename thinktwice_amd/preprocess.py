"""GPU camera preprocessing -- host-side mirror of the image pipeline
(IDAImageTransform + img_transform + ImageTransformMulti:
open_loop_training/code/datasets/pipelines/transform.py:222-378,140-166), one fused kernel per call: `ImagePreprocessor` for
the evaluation branch (is_train=False), `IdaSampler` / `TrainImagePipeline` / `fill_batch` for the training branch
(is_train=True: a resize, crop and flip of its own for every camera of a sample, applied to its depth / seg labels too;
with `augment`, ImageTransformMulti(aug=True)'s colour augmentation of photometric.py in the same pass)."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, calib, ops, photometric
from .ops import check, lib, ptr


class ImagePreprocessor:
    def __init__(self, final_dim=(calib.FINAL_H, calib.FINAL_W), device="cuda", undistort=True):
        self.device = torch.device(device)
        self.final_dim = tuple(final_dim)
        H, W = calib.IMG_H, calib.IMG_W
        fh, fw = self.final_dim
        resize = max(fh / H, fw / W)                       # sample_ida_augmentation, eval branch (transform.py:264-273)
        self.resized = (int(H * resize), int(W * resize))
        self.crop = (self.resized[0] - fh, int(max(0, self.resized[1] - fw) / 2))
        if undistort:
            mx, my = calib.undistort_rectify_map(W, H)
        else:   # identity map: pixel centres (the -0.5 of align_corners=False is applied in the kernel)
            import numpy as np
            mx = np.broadcast_to(np.arange(W, dtype=np.float32)[None] + 0.5, (H, W)).copy()
            my = np.broadcast_to(np.arange(H, dtype=np.float32)[:, None] + 0.5, (H, W)).copy()
        self.mapx = torch.from_numpy(mx).to(self.device).contiguous()
        self.mapy = torch.from_numpy(my).to(self.device).contiguous()
        self.mean = (ctypes.c_float * 3)(*calib.IMAGENET_MEAN)
        self.std = (ctypes.c_float * 3)(*calib.IMAGENET_STD)

    def __call__(self, raw, channel_last_dtype=None, c_pad=None):
        """raw uint8 (..., 900, 1600, 3) on device -> f32 (..., 3, fh, fw) like the reference pipeline, or, with
        `channel_last_dtype`, the channel-last padded tensor (NI, fh, fw, c_pad) the LSS trunk consumes."""
        _lib.require_cuda(raw)
        assert raw.dtype == torch.uint8 and raw.shape[-1] == 3 and raw.is_contiguous()
        lead = raw.shape[:-3]
        H, W = raw.shape[-3], raw.shape[-2]
        NI = 1
        for d in lead:
            NI *= d
        fh, fw = self.final_dim
        nchw = nhwc = None
        if channel_last_dtype is None:
            nchw = torch.empty(NI, 3, fh, fw, dtype=torch.float32, device=raw.device)
            cp, code = 3, _lib.TT_F32
        else:
            cp = c_pad or (4 if channel_last_dtype == torch.float32 else 8)
            nhwc = torch.empty(NI, fh, fw, cp, dtype=channel_last_dtype, device=raw.device)
            code = ops.dtype_code(nhwc)
        check(lib().tt_preprocess_images(ptr(raw), NI, H, W, ptr(self.mapx), ptr(self.mapy), self.resized[0], self.resized[1],
                                         self.crop[0], self.crop[1], fh, fw, self.mean, self.std, ptr(nhwc), cp, code,
                                         ptr(nchw), ops.cur_stream(raw.device)), "tt_preprocess_images")
        if nchw is not None:
            return nchw.view(*lead, 3, fh, fw)
        return nhwc


# one camera's draw of sample_ida_augmentation (transform.py:248-273): `resize` goes into ida_mats, the ints into the kernel
IdaParams = collections.namedtuple("IdaParams", "resize resized_h resized_w crop_y crop_x flip")


IdaSet = _lib.structs()["tt_ida_set"]


class IdaSampler:
    """sample_ida_augmentation's training branch (transform.py:252-263) draw for draw on a numpy RandomState: with
    RandomState(seed) it yields what the reference yields after np.random.seed(seed)."""

    def __init__(self, ida_aug_conf, seed=None):
        self.conf = dict(ida_aug_conf)
        self.rng = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)

    def sample_camera(self):
        c, rng = self.conf, self.rng
        H, W = c["H"], c["W"]
        fH, fW = c["final_dim"]
        resize = rng.uniform(*c["resize_lim"])
        newW, newH = int(W * resize), int(H * resize)
        crop_h = int((1 - rng.uniform(*c["bot_pct_lim"])) * newH) - fH      # (drawn even for limits (0, 0))
        crop_w = int(rng.uniform(0, max(0, newW - fW)))
        flip = bool(c["rand_flip"] and rng.choice([0, 1]))
        return IdaParams(float(resize), newH, newW, crop_h, crop_w, flip)

    def sample(self, batch_size, num_cams=4):
        """[batch_size][num_cams] IdaParams, in the order a loader calling IDAImageTransform once per sample draws them."""
        return [[self.sample_camera() for _ in range(num_cams)] for _ in range(batch_size)]


def ida_mat(params, final_dim):
    """The 4x4 f32 matrix img_transform builds for one draw (transform.py:346-378, rotate = 0)."""
    fw = final_dim[1]
    m = np.eye(4, dtype=np.float32)
    m[0, 0] = -np.float32(params.resize) if params.flip else np.float32(params.resize)
    m[1, 1] = np.float32(params.resize)
    m[0, 3] = float(params.crop_x + fw) if params.flip else -float(params.crop_x)
    m[1, 3] = -float(params.crop_y)
    return m


def check_ida_params(params, final_dim):
    """ValueError for a draw the kernel cannot apply: the crop window must lie inside the resized image."""
    fh, fw = final_dim
    for b, per_cam in enumerate(params):
        for n, p in enumerate(per_cam):
            if p.resized_h <= 0 or p.resized_w <= 0:
                raise ValueError(f"sample {b} camera {n}: resized size {p.resized_h} x {p.resized_w} is not positive")
            if p.crop_y < 0 or p.crop_x < 0 or p.crop_y + fh > p.resized_h or p.crop_x + fw > p.resized_w:
                raise ValueError(f"sample {b} camera {n}: crop ({p.crop_y}, {p.crop_x}) + {fh} x {fw} leaves the resized image "
                                 f"{p.resized_h} x {p.resized_w}")


class TrainImagePipeline(ImagePreprocessor):
    """IDAImageTransform(is_train=True) + ImageTransformMulti(aug=False) on the device: one launch for all frames of a batch
    and one per label kind.  `ida_aug_conf` is the config's (configs/thinktwice.py:111-119)."""

    def __init__(self, ida_aug_conf, undistort=True, device="cuda"):
        super().__init__(final_dim=ida_aug_conf["final_dim"], device=device, undistort=undistort)
        self.ida_aug_conf = dict(ida_aug_conf)

    def _table(self, params, B, N):
        if len(params) != B or any(len(p) != N for p in params):
            raise ValueError(f"params must be [{B}][{N}] IdaParams")
        if B * N > _lib.TT_IDA_MAX_SETS:
            raise ValueError(f"{B} x {N} parameter sets in one call: at most {_lib.TT_IDA_MAX_SETS}")
        check_ida_params(params, self.final_dim)
        flat = [p for per_cam in params for p in per_cam]
        return (IdaSet * len(flat))(*[IdaSet(p.resized_h, p.resized_w, p.crop_y, p.crop_x, int(bool(p.flip))) for p in flat])

    def __call__(self, raw, depth=None, seg=None, params=None, sampler=None, channel_last_dtype=None, c_pad=None, augment=None,
                 pinned_programs=False):
        """raw uint8 [B, T, N, H, W, 3] on the device; depth / seg f32 [B, N, H, W] (key sweep) or None.  `params`
        ([B][N] IdaParams) override `sampler` (an IdaSampler).  Returns dict(img [B, T, N, 3, fh, fw] f32 -- or, with
        `channel_last_dtype`, the channel-last padded [B*T*N, fh, fw, c_pad] tensor the LSS trunk consumes --, depth / seg
        [B, N, fh, fw] where given, ida_mats [B, T, N, 4, 4] f32 on the host, params).
        `augment` (a photometric.PhotometricSampler, or a list of B compiled photometric.Program) adds
        ImageTransformMulti(aug=True): the frames are truncated to uint8 grey levels and every frame of sample b goes through
        program b before the normalisation; the labels and ida_mats are untouched, and the result gains `programs`.
        `pinned_programs`: upload the programs from page-locked memory without waiting for the stream (see
        photometric.device_programs); the result is the same."""
        if raw.dim() != 6 or raw.dtype != torch.uint8 or raw.shape[-1] != 3 or not raw.is_contiguous():
            raise ValueError("raw must be a contiguous uint8 [B, T, N, H, W, 3] tensor")
        B, T, N, H, W, _ = raw.shape
        if params is None:
            if sampler is None:
                raise ValueError("need `params` or a `sampler`")
            params = sampler.sample(B, N)
        for name, lab in (("depth", depth), ("seg", seg)):
            if lab is not None and (lab.dtype != torch.float32 or tuple(lab.shape) != (B, N, H, W) or not lab.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous f32 [{B}, {N}, {H}, {W}] tensor")
        table = self._table(params, B, N)               # (nothing has been launched before this line)
        fh, fw = self.final_dim
        programs = None
        if augment is not None:
            programs = augment.programs(B, fh, fw) if isinstance(augment, photometric.PhotometricSampler) else list(augment)
            photometric.check_programs(programs, B, fh, fw)
        if (H, W) != tuple(self.mapx.shape):            # (the kernels read the map unchecked at raw-image coordinates)
            raise ValueError(f"raw frames are {H} x {W}, the undistortion map {tuple(self.mapx.shape)}")
        _lib.require_cuda(raw, depth, seg)
        stream = ops.cur_stream(raw.device)
        nchw = nhwc = None
        if channel_last_dtype is None:
            nchw = torch.empty(B, T, N, 3, fh, fw, dtype=torch.float32, device=raw.device)
            cp, code = 3, _lib.TT_F32
        else:
            cp = c_pad or (4 if channel_last_dtype == torch.float32 else 8)
            nhwc = torch.empty(B * T * N, fh, fw, cp, dtype=channel_last_dtype, device=raw.device)
            code = ops.dtype_code(nhwc)
        if programs is None:
            check(lib().tt_preprocess_images_ida(ptr(raw), B, T, N, H, W, ptr(self.mapx), ptr(self.mapy), table, fh, fw, self.mean,
                                                 self.std, ptr(nhwc), cp, code, ptr(nchw), stream), "tt_preprocess_images_ida")
        else:
            host, dev, scratch, nbytes = photometric.device_programs(programs, B * T * N, fh, fw, raw.device, pinned_programs)
            check(lib().tt_preprocess_images_ida_aug(ptr(raw), B, T, N, H, W, ptr(self.mapx), ptr(self.mapy), table, fh, fw,
                                                     self.mean, self.std, ptr(nhwc), cp, code, ptr(nchw), host.data_ptr(), ptr(dev),
                                                     ptr(scratch), nbytes, stream), "tt_preprocess_images_ida_aug")
        out = {"img": nchw if nhwc is None else nhwc, "params": params}
        if programs is not None:
            out["programs"] = programs
        for name, lab in (("depth", depth), ("seg", seg)):
            if lab is not None:
                out[name] = torch.empty(B, N, fh, fw, dtype=torch.float32, device=raw.device)
                check(lib().tt_preprocess_labels_ida(ptr(lab), B, N, H, W, ptr(self.mapx), ptr(self.mapy), table, fh, fw,
                                                     ptr(out[name]), stream), "tt_preprocess_labels_ida")
        mats = np.stack([np.stack([ida_mat(p, self.final_dim) for p in per_cam]) for per_cam in params])      # [B, N, 4, 4]
        out["ida_mats"] = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(mats[:, None], (B, T, N, 4, 4))))
        return out


def fill_batch(batch, out):
    """Hand a TrainImagePipeline result to a `forward_train` batch: img, depth, seg and every img_metas[b][t]["ida_mats"]
    (what IDAImageTransform.__call__ writes into the queue, transform.py:328-340)."""
    if out["img"].dim() != 6:
        raise ValueError("fill_batch takes the [B, T, N, 3, fh, fw] form of `img`")
    batch["img"] = out["img"]
    for k in ("depth", "seg"):
        if k in out:
            batch[k] = out[k]
    for b, per_sweep in enumerate(batch["img_metas"]):
        for t, meta in enumerate(per_sweep):
            meta["ida_mats"] = out["ida_mats"][b, t].clone()
    return batch
