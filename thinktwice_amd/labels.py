"""The two label inputs of the training image pipeline from the dataset's raw bytes, on the device: LoadDepth.__call__ and
LoadSeg.__call__ with red_green_yellow (open_loop_training/code/datasets/pipelines/loading.py:84-93, :96-113, :132-162).  The
host side: the class map, the thresholds and the HSV division tables of tt_seg_decode_conf (include/thinktwice_hip.h); the
kernels (csrc/labels.hip) execute them.  The PNG files themselves are decoded by png.py (union2one's merge: sweeps.py).

    decoder = labels.RawLabelDecoder(cfg.seg_label_idxs)
    depth, seg = decoder(raw, depth_rgb_u8, seg_tags_u8)       # raw [B, T, N, H, W, 3], [B, N, H, W, 3], [B, N, H, W], uint8
    out = pipeline(raw, depth, seg, sampler=sampler)           # preprocess.TrainImagePipeline, unchanged

[3P] unpinned.  cv2 was not installed where this was written, so no fixture pins `cv2.cvtColor(..., COLOR_RGB2HSV)` on uint8.
The convention adopted (OpenCV 4.x's integer path RGB2HSV_b, H in 0..179) lives in ONE host function, `hsv_tables`, with its
twin in tests/labels_ref.py; a session that has cv2 can pin it by editing those two and nothing else."""
import ctypes

import numpy as np

from . import _lib, ops
from .ops import check, lib, ptr

TRAFFIC_LIGHT_TAG = 18          # CARLA's semantic tag, literal in loading.py:140
MIN_LIGHT_PIXELS = 20           # loading.py:153
VAL_LOW = 140                   # loading.py:100
GREEN_HUE = (70, 100)           # loading.py:102-103
RED_HUE = (150, 180)            # loading.py:106-107


HsvTables, SegDecodeConf = _lib.structs()["tt_hsv_tables"], _lib.structs()["tt_seg_decode_conf"]


def hsv_tables():
    """(sdiv, hdiv), int32 [256] each: the division tables of OpenCV 4.x's 8-bit RGB -> HSV (RGB2HSV_b, hsv_shift = 12, hue
    range 180): sdiv[i] = rint(255 * 4096 / i), hdiv[i] = rint(180 * 4096 / (6 i)), in f64 with ties to even, entry 0 = 0.
    The single owner of the cv2 convention ([3P] unpinned, see the module docstring)."""
    i = np.arange(1, 256, dtype=np.float64)
    sdiv, hdiv = np.zeros(256, dtype=np.int32), np.zeros(256, dtype=np.int32)
    sdiv[1:] = np.rint((255 << 12) / i)
    hdiv[1:] = np.rint((180 << 12) / (6.0 * i))
    return sdiv, hdiv


def seg_decode_conf(seg_label_idxs, traffic_light_tag=TRAFFIC_LIGHT_TAG):
    """tt_seg_decode_conf of a config's `seg_label_idxs` (configs/thinktwice.py:108): every tag maps to its position in the
    list (so the list's first tag shares class 0 with the background); `traffic_light_tag`, where the list has it, is split
    into components and classified as position + light_type.  None, or a tag the list does not have: no traffic lights."""
    tags = list(seg_label_idxs)
    if any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= t <= 255 for t in tags):
        raise ValueError(f"seg_label_idxs must be integer tags in 0..255, got {tags}")
    if len(set(tags)) != len(tags):
        raise ValueError(f"seg_label_idxs has a tag twice: {tags}")
    if traffic_light_tag is not None and not 0 <= traffic_light_tag <= 255:
        raise ValueError(f"traffic_light_tag {traffic_light_tag} outside 0..255")
    conf = SegDecodeConf()
    conf.light_tag, conf.light_base = -1, 0
    for idx, tag in enumerate(tags):
        if tag == traffic_light_tag:
            if idx > 253:
                raise ValueError(f"the traffic-light tag is entry {idx} of seg_label_idxs: its classes must fit 0..255")
            conf.light_tag, conf.light_base = int(tag), idx
        else:
            conf.class_of_tag[tag] = idx
    conf.min_pixels, conf.val_low = MIN_LIGHT_PIXELS, VAL_LOW
    (conf.green_lo, conf.green_hi), (conf.red_lo, conf.red_hi) = GREEN_HUE, RED_HUE
    for avg in range(256):
        conf.sat_low_of_avg[avg] = int(avg * 1.1)               # loading.py:99, in Python floats as there
    sdiv, hdiv = hsv_tables()
    conf.hsv.sdiv[:] = sdiv.tolist()
    conf.hsv.hdiv[:] = hdiv.tolist()
    return conf


def _require_u8(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError(f"{what} must be a uint8 tensor")
    if not t.is_cuda:
        raise ValueError(f"{what} must be on the device")
    if t.numel() == 0:
        raise ValueError(f"{what} is empty")


def decode_depth(depth_rgb_u8):
    """CARLA depth PNG pixels uint8 [..., H, W, 3] on the device -> metres f32 [..., H, W] (tt_decode_depth_u8)."""
    import torch
    _require_u8(depth_rgb_u8, "depth_rgb_u8")
    if depth_rgb_u8.dim() < 3 or depth_rgb_u8.shape[-1] != 3 or not depth_rgb_u8.is_contiguous():
        raise ValueError("depth_rgb_u8 must be a contiguous uint8 [..., H, W, 3] tensor")
    out = torch.empty(depth_rgb_u8.shape[:-1], dtype=torch.float32, device=depth_rgb_u8.device)
    check(lib().tt_decode_depth_u8(ptr(depth_rgb_u8), out.numel(), ptr(out), ops.cur_stream(out.device)), "tt_decode_depth_u8")
    return out


def rgb2hsv_u8(rgb_u8):
    """uint8 [..., 3] RGB on the device -> uint8 HSV of that shape, H in 0..179 (tt_rgb2hsv_u8 under `hsv_tables`)."""
    import torch
    _require_u8(rgb_u8, "rgb_u8")
    if rgb_u8.dim() < 1 or rgb_u8.shape[-1] != 3 or not rgb_u8.is_contiguous():
        raise ValueError("rgb_u8 must be a contiguous uint8 [..., 3] tensor")
    tab = HsvTables()
    sdiv, hdiv = hsv_tables()
    tab.sdiv[:], tab.hdiv[:] = sdiv.tolist(), hdiv.tolist()
    out = torch.empty_like(rgb_u8)
    check(lib().tt_rgb2hsv_u8(ptr(rgb_u8), rgb_u8.numel() // 3, ctypes.byref(tab), ptr(out), ops.cur_stream(out.device)),
          "tt_rgb2hsv_u8")
    return out


def workspace_bytes(num_images, H, W):
    """tt_decode_seg_workspace_bytes: 24 bytes per pixel (label, count, green, red: 4 each; sum of S: 8)."""
    return num_images * H * W * 24


def decode_seg(tags_u8, rgb_u8, conf, workspace=None):
    """tags uint8 [B, N, H, W] (contiguous) and the RGB frames of the same cameras uint8 [B, N, H, W, 3] -- a view whose
    images are contiguous and whose cameras follow each other, such as raw[:, -1] -- under `conf` (seg_decode_conf) ->
    class ids f32 [B, N, H, W] (tt_decode_seg_u8).  The workspace comes from torch's allocator unless one is handed in (a
    uint8 device tensor of at least workspace_bytes(B * N, H, W))."""
    import torch
    _require_u8(tags_u8, "tags_u8")
    _require_u8(rgb_u8, "rgb_u8")
    if not isinstance(conf, SegDecodeConf):
        raise ValueError("conf must be a labels.SegDecodeConf (seg_decode_conf(seg_label_idxs))")
    if tags_u8.dim() != 4 or not tags_u8.is_contiguous():
        raise ValueError("tags_u8 must be a contiguous uint8 [B, N, H, W] tensor")
    B, N, H, W = tags_u8.shape
    if tuple(rgb_u8.shape) != (B, N, H, W, 3):
        raise ValueError(f"rgb_u8 must be [{B}, {N}, {H}, {W}, 3], got {tuple(rgb_u8.shape)}")
    if rgb_u8.device != tags_u8.device:
        raise ValueError("tags_u8 and rgb_u8 are on different devices")
    if H * W > 2 ** 31 - 1:
        raise ValueError(f"{H} x {W} pixels per image, at most 2^31 - 1")
    if B * N > 65535:
        raise ValueError(f"{B} x {N} images in one call, at most 65535")
    inner = (N * H * W * 3, H * W * 3, W * 3, 3, 1)
    strides = rgb_u8.stride()
    if any(rgb_u8.shape[d] > 1 and strides[d] != inner[d] for d in range(1, 5)) or (B > 1 and strides[0] < inner[0]):
        raise ValueError("rgb_u8: every sample's [N, H, W, 3] block must be contiguous (only the sample stride may be larger)")
    need = workspace_bytes(B * N, H, W)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=tags_u8.device)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != tags_u8.device
          or not workspace.is_contiguous() or workspace.numel() < need):
        raise ValueError(f"workspace must be a contiguous uint8 tensor of at least {need} bytes on the tags' device")
    out = torch.empty(B, N, H, W, dtype=torch.float32, device=tags_u8.device)
    check(lib().tt_decode_seg_u8(ptr(tags_u8), B, N, H, W, ptr(rgb_u8), (strides[0] if B > 1 else inner[0]), ctypes.byref(conf),
                                 ptr(workspace), workspace.numel(), ptr(out), ops.cur_stream(out.device)), "tt_decode_seg_u8")
    return out


class RawLabelDecoder:
    """LoadDepth + LoadSeg of one batch on the device: `(raw, depth_rgb_u8, seg_tags_u8) -> (depth, seg)`, both f32
    [B, N, H, W], ready for `TrainImagePipeline(raw, depth, seg, ...)`.  The traffic lights are classified on the key
    sweep raw[:, -1], read in place."""

    def __init__(self, seg_label_idxs, traffic_light_tag=TRAFFIC_LIGHT_TAG):
        self.conf = seg_decode_conf(seg_label_idxs, traffic_light_tag)

    def __call__(self, raw, depth_rgb_u8, seg_tags_u8):
        _require_u8(raw, "raw")
        if raw.dim() != 6 or raw.shape[-1] != 3 or not raw.is_contiguous():
            raise ValueError("raw must be a contiguous uint8 [B, T, N, H, W, 3] tensor")
        B, T, N, H, W, _ = raw.shape
        _require_u8(depth_rgb_u8, "depth_rgb_u8")
        _require_u8(seg_tags_u8, "seg_tags_u8")
        if tuple(depth_rgb_u8.shape) != (B, N, H, W, 3) or not depth_rgb_u8.is_contiguous():
            raise ValueError(f"depth_rgb_u8 must be a contiguous uint8 [{B}, {N}, {H}, {W}, 3] tensor")
        if tuple(seg_tags_u8.shape) != (B, N, H, W) or not seg_tags_u8.is_contiguous():
            raise ValueError(f"seg_tags_u8 must be a contiguous uint8 [{B}, {N}, {H}, {W}] tensor")
        if depth_rgb_u8.device != raw.device or seg_tags_u8.device != raw.device:
            raise ValueError("raw, depth_rgb_u8 and seg_tags_u8 must be on one device")
        seg = decode_seg(seg_tags_u8, raw[:, -1], self.conf)          # (its size limits are checked before any launch)
        return decode_depth(depth_rgb_u8), seg
