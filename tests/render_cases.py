"""The display lists tt_render_u8 is checked with, shared by the host checker (tests/test_render_host.py, through `write_case_file`)
and the device tests (tests/test_render.py).  `cases(device)` builds every list on `device` out of ONE arena tensor per case, so
that a pointer of the list is `arena address + offset` and the case file can carry the offsets.

Shapes are the smallest at which each rule can go wrong: canvases 40 x 72, 33 x 65 and 7 x 130 (widths off the wave size, odd; 60 x
272 where two column tiles are wanted), a camera tile of 32 x 64 with seg logits 16 x 32 (12 classes in rows of 16, the padding
holding +1e30 and NaN) and depth logits 2 x 4 (80 bins)."""
import collections
import functools
import struct

import numpy as np
import torch

from thinktwice_amd import _lib, render

Case = collections.namedtuple("Case", "name dl arena expect_error")
CANVASES = ((40, 72), (33, 65), (7, 130))
IDENT16 = [[16.0, 0.0, 0.0], [0.0, 16.0, 0.0]]                 # source units = canvas pixels
GUARD = 64
Item = _lib.structs()["tt_render_item"]
PTR_OFFSETS = (Item.src.offset, Item.aux.offset)


class Arena:
    """One uint8 tensor on `device`; `put(array)` copies a numpy array in at the next 256-byte boundary (+ `skew` bytes, a multiple
    of the element size, to take a source off the 16-byte grid) and returns the view.  `live` lists what was handed out."""

    def __init__(self, device, size=1 << 19):
        self.blob = torch.zeros(size, dtype=torch.uint8, device=device)
        self.at, self.live = 256, []

    def put(self, array, skew=0):
        a = np.ascontiguousarray(array)
        start = self.at + skew
        self.at = (start + max(a.nbytes, 1) + 511) // 256 * 256           # at least 256 bytes between two sources
        assert self.at <= self.blob.numel()
        self.live.append((start, a.nbytes))
        view = self.blob[start:start + a.nbytes]
        view.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))
        kinds = {"float32": torch.float32, "uint8": torch.uint8}
        return view.view(kinds[a.dtype.name]).reshape(a.shape)

    def side(self):
        return {"font": self.put(render.font_table()), "palette": self.put(render.seg_palette().reshape(-1)),
                "depth": self.put(render.depth_lut().reshape(-1)), "height": self.put(render.height_lut().reshape(-1))}


# ------------------------------------------------------------------------------------------------------------------- sources
def camera_tile(rng):
    """(3, 32, 64) f32 in network units, with values that land on .5, below 0, above 255, and a NaN."""
    mean, std = np.array(render.calib_mean_std()[0], np.float32), np.array(render.calib_mean_std()[1], np.float32)
    pix = rng.integers(0, 256, (3, 32, 64)).astype(np.float32)
    img = (pix / np.float32(255) - mean[:, None, None]) / std[:, None, None]
    img[0, 3, 5] = np.nan
    img[1, 4, 6] = np.inf
    img[2, 5, 7] = -np.inf
    img[:, 6, 8] = 40.0                                              # far above 255
    img[:, 7, 9] = -40.0                                             # far below 0
    return img.astype(np.float32)


def halves_tile():
    """(3, 8, 16) f32 shown with std = 1 / 255, mean = 0 (so the item's factors are 1 and 0): the values themselves are rounded."""
    v = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -3.0, 254.5, 255.5, 300.0, np.nan, 127.49999, 127.5, 128.5, -0.0, 1e30, -1e30], np.float32)
    return np.stack([np.tile(v, (8, 1)), np.tile(v[::-1], (8, 1)), np.tile(np.roll(v, 3), (8, 1))]).astype(np.float32)


def seg_logits(rng):
    """(16, 32, 16): 12 classes; the padding channels hold +1e30 and NaN and must never be read."""
    z = rng.standard_normal((16, 32, 16)).astype(np.float32)
    z[:, :, :12] += 3 * (rng.integers(0, 12, (16, 32, 1)) == np.arange(12))
    z[:, :, 12:14] = 1e30
    z[:, :, 14:] = np.nan
    z[2, 3, :12] = 1.0                                               # a tie of all: class 0 (the background, left alone)
    z[2, 4, :12] = 0.0
    z[2, 4, [5, 9]] = 7.0                                            # a tie of two: class 5
    z[3, 3, 7] = np.nan                                              # a NaN cell
    z[3, 4, :12] = -np.inf                                           # all -inf: class 0
    z[3, 5, 11] = np.inf
    return z


def depth_logits(rng, stride=80):
    z = rng.standard_normal((2, 4, stride)).astype(np.float32)
    z[:, :, 80:] = np.nan
    z[0, 1, :80] = 2.0                                               # a tie of all: bin 0
    z[0, 2, [17, 60]] = 9.0                                          # a tie of two: bin 17
    z[1, 0, 33] = np.nan                                             # a NaN cell
    z[1, 3, 79] = 50.0                                               # the last bin: LUT index 255
    return z


def _new(device, H, W):
    arena = Arena(device)
    return arena, render.DisplayList(H, W, device, side=arena.side())


# --------------------------------------------------------------------------------------------------------------------- cases
def _scene(device, H, W, dx, dy):
    """Every raster kind once, shifted by (dx, dy): the tiles meet each canvas edge, and some lie wholly outside."""
    rng = np.random.default_rng(11)
    arena, dl = _new(device, H, W)
    cam, seg, dep = arena.put(camera_tile(rng)), arena.put(seg_logits(rng)), arena.put(depth_logits(rng))
    dep_skew = arena.put(depth_logits(rng, 84), skew=4)              # rows off the 16-byte grid: the scalar reads
    rgb, grey = arena.put(rng.integers(0, 256, (24, 40, 3)).astype(np.uint8)), arena.put(rng.integers(0, 256, (24, 40)).astype(np.uint8), skew=1)
    dl.fill(0, 0, W, H, (20, 30, 40))
    dl.image(cam, dx, dy).seg_overlay(seg, dx, dy, factor=2)
    dl.depth_map(dep, dx + 40, dy + 20, scale=8).depth_map(dep_skew, dx - 10, dy + 30, scale=3, bins=80, alpha=160)
    dl.image(rgb, W - 30 + dx, H - 12 + dy).image(rgb, dx + 50, dy - 4, scale=3, alpha=200).image(grey, dx + 2, H - 9, scale=2)
    dl.image(cam, dx + 5, dy + 5, scale=2, w=21, h=13, alpha=128)    # a rectangle smaller than the source gives
    dl.image(cam, 1000, 1000).image(cam, -500, 3).seg_overlay(seg, 5, -400, factor=2)          # wholly outside
    dl.fill(3, 3, 0, 9, (255, 255, 255)).fill(3, 3, 9, 0, (255, 255, 255)).image(cam, 2, 2, w=0, h=5)   # zero-sized
    dl.fill(W - 4, H - 3, 20, 20, (200, 10, 10), alpha=77).fill(-6, -6, 9, 9, (10, 200, 10), alpha=255)
    dl.text("A1/%", W - 14, dy + 1, (255, 255, 0)).text("Z:+-.", -7, H - 5, (0, 255, 255), scale=2, alpha=190)
    return arena, dl


def _overlap(device, order):
    arena, dl = _new(device, 33, 65)
    rng = np.random.default_rng(5)
    rgb = arena.put(rng.integers(0, 256, (20, 30, 3)).astype(np.uint8))
    steps = [lambda: dl.fill(5, 5, 40, 20, (250, 20, 20), alpha=140), lambda: dl.image(rgb, 20, 10, alpha=100),
             lambda: dl.fill(10, 0, 12, 33, (20, 20, 250), alpha=256), lambda: dl.text("OVER", 8, 12, scale=2, alpha=128)]
    for i in (range(4) if order == "ab" else reversed(range(4))):
        steps[i]()
    return arena, dl


def _halves(device):
    arena, dl = _new(device, 7, 130)
    t = arena.put(halves_tile())
    ones = (1.0 / 255,) * 3
    dl.image(t, 0, 0, scale=1, mean=(0, 0, 0), std=ones).image(t, 16, -1, scale=7, mean=(0, 0, 0), std=ones)
    return arena, dl


def _discs(device, H, W):
    arena, dl = _new(device, H, W)
    for i, (x, y) in enumerate(((0, 0), (W, 0), (0, H), (W, H), (W / 2, H / 2), (0.5, 0.5), (W - 0.5, H - 0.5))):
        dl.polyline(arena.put(np.array([[x, y]], np.float32)), IDENT16, (255, 40 * i, 0), half_width=0, radius=16 * 5 + 3 * i)
    dl.polyline(arena.put(np.array([[9, 9]], np.float32)), IDENT16, (255, 255, 255), half_width=30, radius=0)     # no disc, no segment
    dl.polyline(arena.put(np.array([[20.5, 3.5]], np.float32)), IDENT16, (255, 255, 255), half_width=0, radius=1)   # exactly one centre
    return arena, dl


SEGMENTS = (((3, 5), (60, 5)), ((10, 2), (10, 30)), ((20, 1), (26, 31)), ((2, 20), (66, 27)), ((30, 15), (30, 15)),
            ((40.5, 10.5), (47.5, 10.5)), ((-9, -4), (15, 38)), ((50, 35), (200, -60)))


def _segments(device, reverse, half_width):
    """Horizontal, vertical, steep, shallow, zero-length, through pixel centres, leaving the canvas: A -> B, or B -> A."""
    arena, dl = _new(device, 40, 72)
    for a, b in SEGMENTS:
        pts = np.array([b, a] if reverse else [a, b], np.float32)
        dl.polyline(arena.put(pts), IDENT16, (255, 255, 255), half_width=half_width, radius=0)
    return arena, dl


def _bad_points(device):
    arena, dl = _new(device, 33, 65)
    pts = np.array([[5, 5], [np.nan, 7], [30, 9], [40, np.inf], [50, 20], [1e30, 3], [60, 30], [10, 30], [-70000, 12], [65537, 2],
                    [12, 28], [20, 20]], np.float32)                 # 2^20 / 16 = 65536: [65537, 2] is beyond, [-70000, 12] too
    dl.polyline(arena.put(pts), IDENT16, (0, 255, 0), half_width=12, radius=24)
    dl.polyline(arena.put(np.array([[65536, 5], [3, 5]], np.float32)), IDENT16, (255, 0, 0), half_width=8, radius=0)   # on the limit: kept
    dl.marker("cross", (30.0, 16.0), (6.0, 4.0), IDENT16, (255, 255, 0), half_width=8)
    dl.marker("box", (32.0, 16.0), (20.0, 9.0), IDENT16, (0, 255, 255), half_width=6, radius=20, clip=(10, 4, 40, 20))
    dl.marker("box", (3e38, 16.0), (3e38, 9.0), IDENT16, (9, 9, 9))                                                   # cx + hx overflows
    dl.marker("cross", (1e6, 0.0), (1.0, 1.0), IDENT16, (9, 9, 9)).polyline(arena.put(np.zeros((0, 2), np.float32)), IDENT16, (1, 2, 3))
    dl.polyline(arena.put(np.array([[np.nan, np.nan]], np.float32)), IDENT16, (1, 2, 3), clip=(500, 500, 4, 4))      # counted though outside
    return arena, dl


def _clouds(device, H, W):
    arena, dl = _new(device, H, W)
    rng = np.random.default_rng(3)
    pile = np.zeros((500, 4), np.float32)                            # 500 points on one pixel with distinct heights
    pile[:, 0], pile[:, 1], pile[:, 2] = 12.3, 9.6, rng.permutation(500) * 0.01 - 1.0
    x0, y0, w, h = 4, 2, 50, 28
    edges = np.array([[x0, y0, 1], [x0 + w - 0.01, y0 + h - 0.01, 2], [x0 + w, y0 + 5, 3], [x0 + 5, y0 + h, 3], [x0 - 0.01, y0 + 5, 3],
                      [x0 + 5, y0 - 0.01, 3], [x0, y0 + h - 1, 0.5], [x0 + w - 1, y0, 100.0], [x0 + 1, y0 + 1, -100.0]], np.float32)
    edges = np.concatenate([edges, np.zeros((len(edges), 1), np.float32)], 1)
    bad = np.array([[np.nan, 5, 1, 0], [5, np.inf, 1, 0], [7, 7, np.nan, 0], [7, 8, -np.inf, 0], [1e30, 5, 1, 0], [0, 0, 0, 0], [0, 0, 0, 9],
                    [0, 0, 0.5, 0], [-1e9, 3, 1, 0]], np.float32)
    spread = np.concatenate([rng.uniform(-5, 80, (300, 2)), rng.uniform(-3, 7, (300, 1)), np.zeros((300, 1))], 1).astype(np.float32)
    cloud = np.concatenate([pile, edges, bad, spread, np.zeros((40, 4), np.float32)])
    dl.fill(0, 0, W, H, (5, 5, 5))
    dl.points_bev(arena.put(cloud), x0, y0, w, h, IDENT16)
    dl.points_bev(arena.put(cloud[:, :3].copy(), skew=4), W - 20, H - 10, 30, 30, [[8.0, 0, 16.0 * (W - 20)], [0, 8.0, 16.0 * (H - 10)]], alpha=200)
    dl.points_bev(arena.put(np.zeros((0, 4), np.float32)), 0, 0, 10, 10, IDENT16)                                   # n = 0
    dl.points_bev(arena.put(cloud), 1000, 0, 8, 8, IDENT16).points_bev(arena.put(cloud), 0, 0, 0, 5, IDENT16)       # outside; zero-sized
    return arena, dl


def _glyphs(device):
    arena, dl = _new(device, 60, 272)
    chars = "".join(render.GLYPH_CHARS) + "~"                        # every glyph, then a character outside the set
    dl.text(chars, 1, 0).text(chars[:22], 2, 9, (255, 200, 0), scale=2).text(chars[22:], 2, 26, (0, 200, 255), scale=2)
    dl.text("abc xyz \x00\xff", 3, 43, (200, 255, 200)).text("", 5, 52).text("CLIPPED AT THE RIGHT EDGE", 200, 51, scale=1)
    return arena, dl


def _long(device, n):
    """`n` items of every host-only kind, many on each tile: n = 3 chunks, and a count that ends inside a chunk."""
    arena, dl = _new(device, 33, 65)
    rng = np.random.default_rng(n)
    pts = arena.put(rng.uniform(-5, 70, (6, 2)).astype(np.float32))
    while len(dl) < n:
        i = len(dl)
        x, y = int(rng.integers(-8, 65)), int(rng.integers(-8, 33))
        color = tuple(int(v) for v in rng.integers(0, 256, 3))
        if i % 4 == 0:
            dl.fill(x, y, int(rng.integers(0, 30)), int(rng.integers(0, 20)), color, alpha=int(rng.integers(0, 257)))
        elif i % 4 == 1:
            dl.marker("box" if i % 8 == 1 else "cross", (x, y), (7, 4), IDENT16, color, half_width=int(rng.integers(0, 30)), alpha=180)
        elif i % 4 == 2:
            dl.text("%d" % i, x, y, color)
        else:
            dl.polyline(pts[i % 3:i % 3 + 3], IDENT16, color, half_width=6, radius=14, alpha=220)
    return arena, dl


def _errors(device):
    """(name, arena, dl) of lists the entry must refuse."""
    out = []
    rng = np.random.default_rng(2)

    def base():
        arena, dl = _new(device, 33, 65)
        cam, seg = arena.put(camera_tile(rng)), arena.put(seg_logits(rng))
        dl.image(cam, 0, 0).seg_overlay(seg, 0, 0).points_bev(arena.put(np.ones((4, 4), np.float32)), 0, 0, 8, 8, IDENT16).text("X", 1, 1)
        return arena, dl
    for name, patch in (("null_src", lambda d: setattr(d.items[0], "src", None)), ("null_aux", lambda d: setattr(d.items[1], "aux", None)),
                        ("wider_than_source", lambda d: setattr(d.items[0], "w", 65)), ("taller_than_seg", lambda d: setattr(d.items[1], "h", 33)),
                        ("stride_below_classes", lambda d: setattr(d.items[1], "stride", 11)), ("scale_zero", lambda d: setattr(d.items[0], "scale", 0)),
                        ("alpha_257", lambda d: setattr(d.items[0], "alpha", 257)), ("unknown_kind", lambda d: setattr(d.items[0], "kind", 9)),
                        ("plane_misplaced", lambda d: setattr(d.items[2], "ws_offset", 512)), ("negative_width", lambda d: setattr(d.items[0], "w", -1)),
                        ("text_wider_than_run", lambda d: setattr(d.items[3], "w", 7))):
        arena, dl = base()
        patch(dl)
        out.append(("error_" + name, arena, dl))
    arena, dl = _new(device, 33, 65)
    for i in range(_lib.TT_RENDER_MAX_ITEMS + 1):
        dl.fill(i % 60, i % 30, 3, 3, (i % 256, 0, 0))
    out.append(("error_one_over_max_items", arena, dl))
    return out


@functools.lru_cache(maxsize=None)
def cases(device="cpu"):
    out = []

    def add(name, pair, expect_error=False):
        out.append(Case(name, pair[1], pair[0], expect_error))
    for H, W in CANVASES:
        for dx, dy in ((2, 1), (-9, -6), (W - 40, H - 20)):
            add(f"scene_{H}x{W}_at_{dx}_{dy}", _scene(device, H, W, dx, dy))
        add(f"discs_{H}x{W}", _discs(device, H, W))
        add(f"clouds_{H}x{W}", _clouds(device, H, W))
    add("overlap_ab", _overlap(device, "ab"))
    add("overlap_ba", _overlap(device, "ba"))
    add("halves", _halves(device))
    for hw in (0, 8, 23):
        add(f"segments_fwd_hw{hw}", _segments(device, False, hw))
        add(f"segments_rev_hw{hw}", _segments(device, True, hw))
    add("bad_points", _bad_points(device))
    add("glyphs", _glyphs(device))
    add("empty_list", _new(device, 7, 130))
    add("long_3_chunks", _long(device, 3 * _lib.TT_RENDER_CHUNK))
    add("long_3_chunks_and_5", _long(device, 3 * _lib.TT_RENDER_CHUNK + 5))
    add("max_items", _long(device, _lib.TT_RENDER_MAX_ITEMS))
    for name, arena, dl in _errors(device):
        out.append(Case(name, dl, arena, True))
    return tuple(out)


def place_table(case):
    """Puts the case's packed table (and text pool) into its arena -> (the ctypes table, the offset of the packed bytes)."""
    dl, arena = case.dl, case.arena
    start = (arena.at + 255) // 256 * 256
    table, raw = dl.pack(arena.blob.data_ptr() + start)
    assert start + len(raw) + 256 <= arena.blob.numel()
    if raw:
        arena.blob[start:start + len(raw)].copy_(torch.from_numpy(np.frombuffer(raw, np.uint8).copy()))
    return table, start, len(raw)


def write_case_file(path):
    """The CPU cases for tools/render_host_check.cpp.  Little endian: 'TTRC', int32 count; per case: int32 name length, the name, int32
    Hc, Wc, num_items, expect_error, int64 workspace bytes, blob bytes, table offset, int32 live regions, (int64 offset, int64 bytes)
    each, the blob.  Every pointer of the table is stored as 1 + its offset in the blob, 0 for null."""
    cs = cases("cpu")
    with open(path, "wb") as f:
        f.write(b"TTRC" + struct.pack("<i", len(cs)))
        for c in cs:
            table, start, nbytes = place_table(c)
            base = c.arena.blob.data_ptr()
            used = start + nbytes + 256
            blob = bytearray(c.arena.blob[:used].numpy().tobytes())
            for i in range(len(c.dl)):
                for off in PTR_OFFSETS:
                    at = start + i * render.ITEM_BYTES + off
                    p, = struct.unpack_from("<Q", blob, at)
                    assert p == 0 or base <= p < base + used, (c.name, i)
                    struct.pack_into("<Q", blob, at, p - base + 1 if p else 0)
            live = c.arena.live + [(start, nbytes)]
            name = c.name.encode()
            f.write(struct.pack("<i", len(name)) + name + struct.pack("<iiii", c.dl.height, c.dl.width, len(c.dl), int(c.expect_error)))
            f.write(struct.pack("<qqqi", c.dl.workspace_bytes(), used, start, len(live)))
            for off, n in live:
                f.write(struct.pack("<qq", off, n))
            f.write(bytes(blob))
    return len(cs)
