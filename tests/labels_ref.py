"""numpy / scipy restatement of the reference's label loaders, LoadDepth.__call__ and LoadSeg.__call__ with red_green_yellow
(open_loop_training/code/datasets/pipelines/loading.py:84-93, :96-113, :132-162): the reference's expressions line for line,
the oracle of thinktwice_amd.labels and of the kernels of csrc/labels.hip.  Golden F19 (tests/golden/README_f19.md) pins
everything here to the reference's own module EXCEPT the three cv2 stand-ins at the bottom.

[3P] unpinned: `rgb2hsv_u8` (with `hsv_tables`, the twin of thinktwice_amd.labels.hsv_tables) restates
cv2.cvtColor(..., COLOR_RGB2HSV) on uint8 from OpenCV 4.x's integer path RGB2HSV_b; cv2 is not installed where this was
written.  `in_range` restates cv2.inRange on uint8 with integer bounds (inclusive; a bound above 255 matches nothing).

One deliberate difference from the reference: `LoadSeg.__call__` drops the FIRST group of its argsort (`[...][1:]`, :150-151),
which is label 0 whenever the image has a pixel that is no traffic light; on an image that is ALL traffic light it drops the
one component instead and then raises IndexError.  Here the dropped group is label 0 where there is one, so that image
gives one classified component."""
import numpy as np
from scipy.ndimage import label as sep_mask


# ------------------------------------------------------------------------------------------------------- loading.py:84-93
def decode_depth(depth_rgb_u8):
    """uint8 [..., 3] -> f32 [...], LoadDepth.__call__'s three lines."""
    rgb = np.asarray(depth_rgb_u8).astype(np.float32)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    depth = (r + g * 256 + b * 256 * 256) / (256 ** 3 - 1) * 1000
    assert depth.dtype == np.float32
    return depth


# ------------------------------------------------------------------------------------------------------ loading.py:96-113
def red_green_yellow(rgb_image, cvt=None, in_rng=None):
    """`rgb_image` uint8 [n, 3], the pixels of one component -> 0 (not sure / yellow), 1 (red), 2 (green)."""
    cvt, in_rng = cvt or rgb2hsv_u8, in_rng or in_range
    hsv = cvt(rgb_image[:, None, :])
    avg_saturation = int(hsv[:, :, 1].mean())
    sat_low = int(avg_saturation * 1.1)
    val_low = 140
    lower_green = np.array([70, sat_low, val_low])
    upper_green = np.array([100, 255, 255])
    sum_green = in_rng(hsv, lower_green, upper_green).astype(np.bool_).sum()
    lower_red = np.array([150, sat_low, val_low])
    upper_red = np.array([180, 255, 255])
    sum_red = in_rng(hsv, lower_red, upper_red).astype(np.bool_).sum()
    if sum_red < 3 and sum_green < 3:
        return 0
    if sum_red >= sum_green:
        return 1
    return 2


# ----------------------------------------------------------------------------------------------------- loading.py:132-162
def components(tl_part):
    """(row_indices, col_indices), one array per 8-connected component of the bool mask, in scipy's label order: :144-151."""
    tl_mask, num_tl = sep_mask(tl_part, structure=[[1, 1, 1], [1, 1, 1], [1, 1, 1]])
    a_flattened = tl_mask.ravel()
    sidx = np.argsort(a_flattened, kind="stable")
    afs = a_flattened[sidx]
    cut_idx = np.r_[0, np.flatnonzero(afs[1:] != afs[:-1]) + 1, a_flattened.size]
    row, col = np.unravel_index(sidx, tl_mask.shape)
    first = 1 if afs.size and afs[0] == 0 else 0            # (the module docstring's difference: the reference has 1)
    row_indices = [row[i:j] for i, j in zip(cut_idx[:-1], cut_idx[1:])][first:]
    col_indices = [col[i:j] for i, j in zip(cut_idx[:-1], cut_idx[1:])][first:]
    assert len(row_indices) == num_tl
    return row_indices, col_indices


def decode_seg(tags_u8, rgb_u8, seg_label_idxs, traffic_light_tag=18, min_pixels=20):
    """One image: tags uint8 [H, W], its RGB frame uint8 [H, W, 3] -> class ids f32 [H, W]."""
    src = np.asarray(tags_u8).astype(np.float32)
    seg = np.zeros_like(src)
    for idx, label in enumerate(seg_label_idxs):
        if label == traffic_light_tag:
            now_img = rgb_u8
            tl_part = src == label
            row_indices, col_indices = components(tl_part)
            for tl_index in range(len(row_indices)):
                if len(row_indices[tl_index]) < min_pixels:
                    continue
                now_tl = now_img[row_indices[tl_index], col_indices[tl_index], :]
                light_type = red_green_yellow(now_tl)
                seg[row_indices[tl_index], col_indices[tl_index]] = idx + light_type
        else:
            seg[np.where(src == label)] = idx
    return seg


def decode_seg_batch(tags_u8, rgb_u8, seg_label_idxs, traffic_light_tag=18):
    """tags [..., H, W], rgb [..., H, W, 3] -> f32 [..., H, W], image by image."""
    tags_u8, rgb_u8 = np.asarray(tags_u8), np.asarray(rgb_u8)
    lead, (H, W) = tags_u8.shape[:-2], tags_u8.shape[-2:]
    t, c = tags_u8.reshape(-1, H, W), rgb_u8.reshape(-1, H, W, 3)
    out = np.stack([decode_seg(t[i], c[i], seg_label_idxs, traffic_light_tag) for i in range(len(t))])
    return out.reshape(*lead, H, W)


# ------------------------------------------------------------------------------------------------ [3P] the cv2 stand-ins
COLOR_RGB2HSV = 41          # cv2's enum value; only its identity matters here


def hsv_tables():
    """OpenCV 4.x RGB2HSV_b: hsv_shift = 12, sdiv_table[i] = saturate_cast<int>((255 << 12) / (1. * i)), hdiv_table180[i] =
    saturate_cast<int>((180 << 12) / (6. * i)), saturate_cast<int>(double) rounding to nearest, ties to even; entry 0 = 0."""
    sdiv, hdiv = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    for i in range(1, 256):
        sdiv[i] = int(np.rint((255 << 12) / (1.0 * i)))
        hdiv[i] = int(np.rint((180 << 12) / (6.0 * i)))
    return sdiv, hdiv


def rgb2hsv_u8(rgb_u8, code=COLOR_RGB2HSV):
    """uint8 [..., 3] RGB -> uint8 [..., 3] HSV, H in 0..179."""
    assert code == COLOR_RGB2HSV
    sdiv, hdiv = hsv_tables()
    px = np.asarray(rgb_u8).astype(np.int64)
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    out = np.stack([h, s, v], axis=-1)
    assert out.min() >= 0 and out.max() <= 255 and h.max() <= 179       # saturate_cast<uchar> never has to saturate
    return out.astype(np.uint8)


def in_range(src_u8, lowerb, upperb):
    """uint8 [..., C] within [lowerb, upperb] on every channel -> uint8 [...] of 255 / 0."""
    src = np.asarray(src_u8).astype(np.int64)
    ok = np.all((src >= np.asarray(lowerb)) & (src <= np.asarray(upperb)), axis=-1)
    return np.where(ok, 255, 0).astype(np.uint8)
