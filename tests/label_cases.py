"""Hand-made inputs of the label-decode tests (test_label_decode.py on the device, test_labels_cpu.py for the restatement):
traffic-light masks that stress a tiled connected-component labelling, and components painted so that the counts of
red_green_yellow (loading.py:96-113) are known.  Data only: every expectation comes from tests/labels_ref.py."""
import functools

import numpy as np

import labels_ref as R

IDXS = [1, 4, 5, 6, 7, 8, 10, 12, 18]           # configs/thinktwice.py:108
TILE_H, TILE_W = 16, 64                         # the tile of csrc/labels.hip's local pass
SIZES = [(37, 53), (64, 64), (65, 129)]         # tile edges inside, on and one past the image's edge


def spiral(H, W):
    """A one-pixel-wide spiral from the corner to the centre, its arms one pixel apart: one component, the longest path."""
    m = np.zeros((H, W), dtype=bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        ahead = 0 <= ny < H and 0 <= nx < W and not m[ny, nx]
        if ahead and 0 <= ny + dy < H and 0 <= nx + dx < W and m[ny + dy, nx + dx]:
            ahead = False                       # keep a pixel between this arm and the one in front
        if ahead:
            y, x, turns = ny, nx, 0
            m[y, x] = True
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return m


def mask_cases(H, W):
    """{name: bool [H, W]}."""
    rng = np.random.default_rng(1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    z = lambda: np.zeros((H, W), dtype=bool)          # noqa: E731
    out = {"empty": z(), "full": ~z(), "checkerboard": (yy + xx) % 2 == 0, "spiral": spiral(H, W),
           "noise": rng.random((H, W)) < 0.2}
    m = z()                                     # serpentine: every second row, joined at alternating ends
    m[::2] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    out["serpentine"] = m
    m = z()                                     # comb: a spine with one-pixel teeth
    m[0] = True
    m[:, ::2] = True
    out["comb"] = m
    m = z()                                     # frame: one component touching all four borders
    m[0] = m[-1] = True
    m[:, 0] = m[:, -1] = True
    out["frame"] = m
    m = z()                                     # nested U shapes: the arms meet only in the last tile row / last tile column
    for k in range(3):
        m[2 + 2 * k:H - 2 - 2 * k, 3 + 4 * k] = m[2 + 2 * k:H - 2 - 2 * k, W // 2 - 2 - 4 * k] = True
        m[H - 3 - 2 * k, 3 + 4 * k:W // 2 - 1 - 4 * k] = True
    for k in range(2):
        m[3 + 4 * k, W // 2 + 2:W - 2 - 2 * k] = m[H - 4 - 4 * k, W // 2 + 2:W - 2 - 2 * k] = True
        m[3 + 4 * k:H - 3 - 4 * k, W - 3 - 2 * k] = True
    out["u shapes"] = m
    # pairs joined only by one diagonal step across a tile edge -- a tile CORNER where the image has a tile column edge --:
    # a 24-pixel bar above the edge, three pixels below it; missing the step leaves the three under the 20-pixel rule
    m = z()
    ey = TILE_H
    ex = TILE_W if W > TILE_W else 28
    m[ey - 1, ex - 24:ex] = True                # ends at (ey - 1, ex - 1); joined to (ey, ex): that pixel's NW neighbour
    m[ey, ex:ex + 3] = True
    ey = 2 * TILE_H
    m[ey - 1, ex:ex + 24 if ex + 24 < W else W] = True      # starts at (ey - 1, ex); joined to (ey, ex - 1): that pixel's NE neighbour
    m[ey, ex - 3:ex] = True
    if W > TILE_W:                              # and sideways: across a tile column edge in the middle of a tile row
        m[40:64 if H >= 64 else H, ex - 1] = True
        m[39, ex:ex + 2] = True                 # (39, ex) is the NE neighbour of (40, ex - 1)
    out["corner diagonals"] = m
    m = z()                                     # two bars one pixel apart, and two that touch only the image's borders
    m[5, 2:32] = m[7, 2:32] = True
    m[20:24, 10:20] = m[25:29, 10:20] = True
    out["one pixel apart"] = m
    m = z()
    m[1, 1:20] = True                           # 19 pixels: stays 0
    m[3, 1:21] = True                           # 20 pixels: classified
    m[17:36, 40] = True                         # 19, across two tile rows
    m[16:36, 44] = True                         # 20, across two tile rows
    out["nineteen and twenty"] = m
    return out


@functools.lru_cache(maxsize=None)
def _hsv_of_all_rgb():
    code = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([code & 255, (code >> 8) & 255, code >> 16], axis=-1).astype(np.uint8)
    hsv = np.concatenate([R.rgb2hsv_u8(rgb[i:i + (1 << 21)]) for i in range(0, 1 << 24, 1 << 21)])
    return rgb, hsv


def rgb_with(h=None, s=None, v=None):
    """An RGB triple whose HSV (under labels_ref's convention) has the given values; a missing one is 'a clearly lit red'
    (H 160..175, S >= 150, V >= 150)."""
    rgb, hsv = _hsv_of_all_rgb()
    ok = np.ones(len(rgb), dtype=bool)
    for c, want, lo, hi in ((0, h, 160, 175), (1, s, 150, 255), (2, v, 150, 255)):
        ok &= (hsv[:, c] == want) if want is not None else ((hsv[:, c] >= lo) & (hsv[:, c] <= hi))
    return rgb[np.flatnonzero(ok)[0]]


GREY = (50, 50, 50)                             # S = 0, V = 50: counts for nothing, lowers the mean saturation


def decision_cases():
    """(tags [1, K, 8, 64], rgb [1, K, 8, 64, 3], {name: light_type}) -- one 40-pixel component per image, painted as
    runs of (count, RGB); the images are in sorted(name) order."""
    red, green = rgb_with(h=170, s=200), rgb_with(h=85, s=200)
    cases = {
        "red 2": ([(2, red), (38, GREY)], 0),
        "red 3": ([(3, red), (37, GREY)], 1),
        "green 3 red 0": ([(3, green), (37, GREY)], 2),
        "green 3 red 2": ([(3, green), (2, red), (35, GREY)], 2),
        "tie 4 4": ([(4, green), (4, red), (32, GREY)], 1),
        # mean S = (20 * 110 + 20 * 90) / 40 = 100 -> sat_low = int(100 * 1.1) = 110
        "S at sat_low": ([(20, rgb_with(s=110)), (20, rgb_with(h=40, s=90))], 1),
        # mean S = (20 * 109 + 20 * 91) / 40 = 100 -> 110 again, one above the painted 109
        "S below sat_low": ([(20, rgb_with(s=109)), (20, rgb_with(h=40, s=91))], 0),
        "V 139": ([(5, rgb_with(v=139)), (35, GREY)], 0),
        "V 140": ([(5, rgb_with(v=140)), (35, GREY)], 1),
        # every pixel S = 240: sat_low = int(240 * 1.1) = 264 > 255, nothing counts although every pixel is a lit red
        "sat_low over 255": ([(40, rgb_with(h=170, s=240))], 0),
    }
    for hue, kind in ((69, 0), (70, 2), (100, 2), (101, 0), (149, 0), (150, 1)):
        cases[f"H {hue:03d}"] = ([(5, rgb_with(h=hue, s=200)), (35, GREY)], kind)
    names = sorted(cases)
    rng = np.random.default_rng(7)
    tags = np.full((1, len(names), 8, 64), 4, dtype=np.uint8)
    rgb = rng.integers(0, 256, (1, len(names), 8, 64, 3), dtype=np.uint8)
    for i, k in enumerate(names):
        runs, _ = cases[k]
        assert sum(n for n, _ in runs) == 40
        tags[0, i, 2, 3:43] = 18
        rgb[0, i, 2, 3:43] = np.concatenate([np.tile(np.asarray(c, dtype=np.uint8), (n, 1)) for n, c in runs])
    return tags, rgb, {k: v[1] for k, v in cases.items()}


def batch_isolation_case():
    """(tags [2, 3, 37, 53], rgb): masks on the last row / last column of one image and the first row / first column of
    the next in memory, whole last and first rows, and the last pixel of an image with the first of the next."""
    B, N, H, W = 2, 3, 37, 53
    rng = np.random.default_rng(11)
    tags = np.full((B * N, H, W), 7, dtype=np.uint8)
    rgb = rng.integers(0, 256, (B, N, H, W, 3), dtype=np.uint8)
    tags[0, H - 1, :] = tags[1, 0, :] = 18                          # 53 + 53 pixels that are neighbours in memory only
    tags[1, H - 1, W - 12:] = 18                                    # 12 pixels ...
    tags[2, 0, :12] = 18                                            # ... and 12: a link across the images would make 24 >= 20
    tags[2, :, W - 1] = tags[3, :, 0] = 18                          # last column, first column (across the sample boundary)
    tags[3, H - 1, W - 1] = tags[4, 0, 0] = 18                      # one pixel each
    tags[4, H - 10:, W - 1] = tags[5, :10, 0] = 18                  # 10 + 10
    tags[5, H - 1, 20:] = 18
    rgb[:, :, 0] = rgb_with(h=170, s=220)                    # first rows red, last rows green: a shared component
    rgb[:, :, H - 1] = rgb_with(h=85, s=220)                 # would also change the colour counts
    return tags.reshape(B, N, H, W), rgb
