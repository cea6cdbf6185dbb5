"""Debug frames drawn on the device: what the model predicted, as a picture the recorder can write.

    dl = render.DisplayList(height, width, device)          # a table of tt_render_item (include/thinktwice_hip.h)
    dl.image(img_f32[0], 0, 0); dl.seg_overlay(seg_logits_cl[0], 0, 0, factor=2); dl.text("STEER", 4, 4)
    canvas = render.Rasteriser(device).draw(dl)             # uint8 (height, width, 3) device tensor: one tt_render_u8

    dbg = render.DebugRenderer(model_cfg, device=model.device)
    frame = dbg.frame(info["img"], info["pred"], info["cloud"], controls={...}, target=info["target_point"])

`DisplayList` holds its tensors by reference: nothing is copied or synchronised when an item is added, and drawing queues one
upload of the table (with the text bytes behind it) and the launches of tt_render_u8 on the current stream.  The per-pixel rules
are csrc/render_raster.h; tests/render_ref.py restates them in numpy.

The palette, the two colour tables, the layout and the 5 x 7 font below are this project's own: the reference draws nothing (its
debug panel is a simulator-side camera, which stays out of scope)."""
import ctypes

import numpy as np

from . import _lib

Item = _lib.structs()["tt_render_item"]
ITEM_BYTES = ctypes.sizeof(Item)
STATUS_BYTES = 256                       # the status words, rounded up as the planes are
NONFINITE = (255, 0, 255)                # the colour of a NaN: magenta, which no table below produces

# ------------------------------------------------------------------------------------------------------------------- the font
# 5 x 7 glyphs, rows top to bottom, '#' = set.  Glyph 0 is the box drawn for every character outside the set.
_GLYPHS = {
    None: "##### #...# #...# #...# #...# #...# #####",
    " ": "..... ..... ..... ..... ..... ..... .....",
    "0": ".###. #...# #..## #.#.# ##..# #...# .###.",
    "1": "..#.. .##.. ..#.. ..#.. ..#.. ..#.. .###.",
    "2": ".###. #...# ....# ...#. ..#.. .#... #####",
    "3": "####. ....# ....# .###. ....# ....# ####.",
    "4": "...#. ..##. .#.#. #..#. ##### ...#. ...#.",
    "5": "##### #.... ####. ....# ....# #...# .###.",
    "6": "..##. .#... #.... ####. #...# #...# .###.",
    "7": "##### ....# ...#. ..#.. .#... .#... .#...",
    "8": ".###. #...# #...# .###. #...# #...# .###.",
    "9": ".###. #...# #...# .#### ....# ...#. .##..",
    "A": ".###. #...# #...# ##### #...# #...# #...#",
    "B": "####. #...# #...# ####. #...# #...# ####.",
    "C": ".###. #...# #.... #.... #.... #...# .###.",
    "D": "###.. #..#. #...# #...# #...# #..#. ###..",
    "E": "##### #.... #.... ####. #.... #.... #####",
    "F": "##### #.... #.... ####. #.... #.... #....",
    "G": ".###. #...# #.... #.### #...# #...# .####",
    "H": "#...# #...# #...# ##### #...# #...# #...#",
    "I": ".###. ..#.. ..#.. ..#.. ..#.. ..#.. .###.",
    "J": "..### ...#. ...#. ...#. ...#. #..#. .##..",
    "K": "#...# #..#. #.#.. ##... #.#.. #..#. #...#",
    "L": "#.... #.... #.... #.... #.... #.... #####",
    "M": "#...# ##.## #.#.# #.#.# #...# #...# #...#",
    "N": "#...# ##..# #.#.# #..## #...# #...# #...#",
    "O": ".###. #...# #...# #...# #...# #...# .###.",
    "P": "####. #...# #...# ####. #.... #.... #....",
    "Q": ".###. #...# #...# #...# #.#.# #..#. .##.#",
    "R": "####. #...# #...# ####. #.#.. #..#. #...#",
    "S": ".#### #.... #.... .###. ....# ....# ####.",
    "T": "##### ..#.. ..#.. ..#.. ..#.. ..#.. ..#..",
    "U": "#...# #...# #...# #...# #...# #...# .###.",
    "V": "#...# #...# #...# #...# #...# .#.#. ..#..",
    "W": "#...# #...# #...# #.#.# #.#.# ##.## #...#",
    "X": "#...# #...# .#.#. ..#.. .#.#. #...# #...#",
    "Y": "#...# #...# .#.#. ..#.. ..#.. ..#.. ..#..",
    "Z": "##### ....# ...#. ..#.. .#... #.... #####",
    ".": "..... ..... ..... ..... ..... .##.. .##..",
    "-": "..... ..... ..... ##### ..... ..... .....",
    "+": "..... ..#.. ..#.. ##### ..#.. ..#.. .....",
    ":": "..... .##.. .##.. ..... .##.. .##.. .....",
    "%": "##..# ##.#. ...#. ..#.. .#... .#.## #..##",
    "/": "....# ....# ...#. ..#.. .#... #.... #....",
}
GLYPH_CHARS = [c for c in _GLYPHS if c is not None]          # glyph number = 1 + position here


def glyph_rows(ch):
    """The 7 row bytes of a character's glyph (bit 4 = the leftmost column); the box for a character outside the set."""
    rows = _GLYPHS.get(ch.upper() if isinstance(ch, str) else ch, _GLYPHS[None]).split()
    return [int(r.replace("#", "1").replace(".", "0"), 2) for r in rows]


def font_table():
    """256 bytes character -> glyph number (lower case shares the capitals' glyphs), then 8 bytes per glyph."""
    table = np.zeros(256 + 8 * (1 + len(GLYPH_CHARS)), np.uint8)
    for g, ch in enumerate([None] + GLYPH_CHARS):
        table[256 + 8 * g:256 + 8 * g + 7] = glyph_rows(ch)
        if ch is not None:
            table[ord(ch)] = g
            table[ord(ch.lower())] = g
    return table


NUM_GLYPHS = 1 + len(GLYPH_CHARS)

# --------------------------------------------------------------------------------------------------------- palette and tables
# One r, g, b, a per seg class as evaluate.seg_class_names numbers them; class 0 is the background and the only alpha 0.
SEG_PALETTE = np.array([
    (0, 0, 0, 0),            # background / building
    (220, 40, 60, 176),      # pedestrian
    (160, 160, 160, 144),    # pole
    (250, 240, 80, 176),     # road line
    (130, 70, 130, 112),     # road
    (240, 40, 230, 112),     # sidewalk
    (40, 90, 230, 176),      # vehicle
    (230, 220, 0, 176),      # traffic sign
    (250, 170, 30, 176),     # traffic light
    (255, 0, 0, 208),        # traffic light, red
    (0, 255, 0, 208),        # traffic light, green
    (0, 200, 200, 144),      # spare class
], np.uint8)


def seg_palette(num_classes=12):
    if num_classes <= len(SEG_PALETTE):
        return SEG_PALETTE[:num_classes].copy()
    extra = [((37 * i) % 256, (91 * i) % 256, (173 * i) % 256, 144) for i in range(len(SEG_PALETTE), num_classes)]
    return np.concatenate([SEG_PALETTE, np.array(extra, np.uint8)])


def depth_lut():
    """Near bins warm, far bins cold: 256 x 3."""
    i = np.arange(256)
    return np.stack([255 - i, 255 - np.abs(2 * i - 255), i], 1).astype(np.uint8)


def height_lut():
    """Low points dark blue, high points towards yellow-white: 256 x 3."""
    i = np.arange(256)
    return np.stack([np.minimum(255, 40 + 2 * i), np.minimum(255, 80 + (3 * i) // 4), 255 - (3 * i) // 4], 1).astype(np.uint8)


STAGE_COLORS = [(90, 90, 255), (60, 170, 255), (60, 230, 200), (120, 240, 90), (250, 220, 60), (255, 110, 40)]

_TABLES = {}


def tables(device):
    """The side tables on `device`, uploaded once per process and device."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _TABLES:
        host = {"font": font_table(), "palette": seg_palette().reshape(-1), "depth": depth_lut().reshape(-1), "height": height_lut().reshape(-1)}
        _TABLES[device] = {k: torch.from_numpy(v.copy()).to(device) for k, v in host.items()}
    return _TABLES[device]


def calib_mean_std():
    """(mean, std) of pixel / 255 as ImagePreprocessor normalises: where the preprocessor keeps them."""
    from . import calib
    return calib.IMAGENET_MEAN, calib.IMAGENET_STD


def _color(c):
    r, g, b = (int(v) for v in c)
    if not all(0 <= v <= 255 for v in (r, g, b)):
        raise ValueError(f"colour {c!r} outside 0..255")
    return r | g << 8 | b << 16


def _up(n, a):
    return (n + a - 1) // a * a


class DisplayList:
    """A canvas size and the items to draw on it, in painter's order.  Every method appends one item (`bar` two or three) and returns
    self.  x, y, w, h are canvas pixels; `alpha` 0..256.  `refs[i]` keeps what item i points at; `text_bytes` is the pool of every
    text run, which travels behind the table (see `pack`)."""

    def __init__(self, height, width, device="cuda", side=None):
        import torch
        self.height, self.width, self.device = int(height), int(width), torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.side = side if side is not None else tables(self.device)       # font, palette, depth, height: uint8 tensors
        self.items, self.refs, self.text_bytes, self._text_at = [], [], bytearray(), {}
        self._plane_at = STATUS_BYTES

    def __len__(self):
        return len(self.items)

    def _add(self, kind, x, y, w, h, refs=(), **fields):
        it = Item()
        it.kind, it.x0, it.y0, it.w, it.h, it.scale, it.alpha = kind, int(x), int(y), int(w), int(h), 1, 256
        for k, v in fields.items():
            if k in ("m", "p"):
                for i, f in enumerate(v):
                    getattr(it, k)[i] = float(f)
            else:
                setattr(it, k, v)
        self.items.append(it)
        self.refs.append(tuple(refs))
        return self

    def _f32(self, t, dims, what):
        import torch
        if not isinstance(t, torch.Tensor) or t.dim() != dims or t.device != self.device:
            raise ValueError(f"{what}: a {dims}-d tensor on {self.device} is needed")
        if t.dtype != torch.float32:
            t = t.float()                                            # (bf16 / f16 storage modes, as MetricWindow reads them)
        return t if t.is_contiguous() else t.contiguous()

    def _table(self, t, n, what):
        import torch
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(t, np.uint8).reshape(-1).copy()).to(self.device)
        if t.dtype != torch.uint8 or t.numel() < n or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"{what}: {n} contiguous uint8 values on {self.device} are needed")
        return t

    def fill(self, x, y, w, h, color, alpha=256):
        return self._add(_lib.TT_RENDER_FILL, x, y, w, h, color=_color(color), alpha=int(alpha))

    def image(self, src, x, y, scale=1, w=None, h=None, mean=None, std=None, alpha=256, nonfinite=NONFINITE):
        """f32 (3, h, w): a network input, shown through mean / std (of pixel / 255; default: the preprocessor's, calib.IMAGENET_*,
        so the item carries 255 std and 255 mean) at `scale` x; uint8 (h, w, 3),
        (h, w, 1) or (h, w): shown 1:1 or reduced by the box factor `scale`."""
        import torch
        if isinstance(src, torch.Tensor) and src.dtype == torch.uint8:
            if src.dim() not in (2, 3) or (src.dim() == 3 and src.shape[2] not in (1, 3)) or src.device != self.device:
                raise ValueError(f"image: uint8 (h, w, 3), (h, w, 1) or (h, w) on {self.device} is needed")
            src = src if src.is_contiguous() else src.contiguous()
            sh, sw, ch = src.shape[0], src.shape[1], (src.shape[2] if src.dim() == 3 else 1)
            return self._add(_lib.TT_RENDER_IMAGE_U8, x, y, sw // scale if w is None else w, sh // scale if h is None else h, (src,),
                             sw=sw, sh=sh, scale=int(scale), channels=ch, alpha=int(alpha), src=src.data_ptr())
        src = self._f32(src, 3, "image")
        if src.shape[0] != 3:
            raise ValueError("image: f32 (3, h, w) is needed")
        mean = calib_mean_std()[0] if mean is None else mean
        std = calib_mean_std()[1] if std is None else std
        sh, sw = src.shape[1], src.shape[2]
        return self._add(_lib.TT_RENDER_IMAGE_F32, x, y, sw * scale if w is None else w, sh * scale if h is None else h, (src,),
                         sw=sw, sh=sh, scale=int(scale), alpha=int(alpha), color=_color(nonfinite), m=[255.0 * v for v in std] + [255.0 * v for v in mean],
                         src=src.data_ptr())

    def _logits(self, kind, logits, x, y, scale, channels, table, w, h, alpha, nonfinite, what):
        t = self._f32(logits, 3, what)
        sh, sw, stride = t.shape
        channels = stride if channels is None else int(channels)
        return self._add(kind, x, y, sw * scale if w is None else w, sh * scale if h is None else h, (t, table), sw=sw, sh=sh,
                         scale=int(scale), channels=channels, stride=stride, alpha=int(alpha), color=_color(nonfinite),
                         src=t.data_ptr(), aux=table.data_ptr())

    def seg_overlay(self, logits_cl, x, y, factor=2, num_classes=12, palette=None, w=None, h=None, nonfinite=NONFINITE):
        """(h / f, w / f, cstride >= num_classes) channel-last logits, argmax through the palette, blended over what is below."""
        table = self.side["palette"] if palette is None else self._table(palette, 4 * num_classes, "palette")
        if table.numel() < 4 * num_classes:
            raise ValueError(f"seg_overlay: the palette has {table.numel() // 4} entries for {num_classes} classes")
        return self._logits(_lib.TT_RENDER_SEG_OVERLAY, logits_cl, x, y, factor, num_classes, table, w, h, 256, nonfinite, "seg_overlay")

    def depth_map(self, logits_cl, x, y, scale=8, bins=None, lut=None, w=None, h=None, alpha=256, nonfinite=NONFINITE):
        """(h / f, w / f, cstride >= bins) channel-last depth logits, argmax bin through a 256-entry colour table."""
        table = self.side["depth"] if lut is None else self._table(lut, 768, "lut")
        return self._logits(_lib.TT_RENDER_DEPTH_MAP, logits_cl, x, y, scale, bins, table, w, h, alpha, nonfinite, "depth_map")

    def points_bev(self, cloud, x, y, w, h, matrix, z_lo=-2.0, z_hi=6.0, lut=None, alpha=256):
        """(n, stride >= 3) f32 cloud through `matrix` (2 x 3: x, y metres -> 1/16 px of the canvas), coloured by height."""
        t = self._f32(cloud, 2, "points_bev")
        if t.shape[0] and t.shape[1] < 3:
            raise ValueError("points_bev: rows of at least 3 floats are needed")
        table = self.side["height"] if lut is None else self._table(lut, 768, "lut")
        inv_step = float(np.float32(256.0) / (np.float32(z_hi) - np.float32(z_lo)))
        at = self._plane_at
        self._plane_at += _up(4 * max(int(w), 0) * max(int(h), 0), 256)
        return self._add(_lib.TT_RENDER_POINTS_BEV, x, y, w, h, (t, table), count=t.shape[0], stride=max(t.shape[1], 3), alpha=int(alpha),
                         m=np.asarray(matrix, np.float32).reshape(6), p=[z_lo, inv_step, 0, 0], ws_offset=at,
                         src=t.data_ptr() if t.shape[0] else None, aux=table.data_ptr())

    def polyline(self, points, matrix, color, half_width=16, radius=40, clip=None, alpha=256):
        """(m, 2) f32 DEVICE points (a row of pred_wp) through `matrix`; widths in 1/16 px; `clip` = (x, y, w, h), default the canvas."""
        t = self._f32(points, 2, "polyline")
        if t.shape[1] != 2 or t.shape[0] > _lib.TT_RENDER_MAX_POINTS:
            raise ValueError(f"polyline: (m, 2) points, m <= {_lib.TT_RENDER_MAX_POINTS}")
        x, y, w, h = clip if clip is not None else (0, 0, self.width, self.height)
        return self._add(_lib.TT_RENDER_POLYLINE_DEV, x, y, w, h, (t,), count=t.shape[0], color=_color(color), alpha=int(alpha),
                         half_width=int(half_width), radius=int(radius), m=np.asarray(matrix, np.float32).reshape(6),
                         src=t.data_ptr() if t.shape[0] else None)

    def marker(self, shape, center, half, matrix, color, half_width=16, radius=0, clip=None, alpha=256):
        """A cross or a box from HOST floats: `center` and `half` extents in the matrix's source units (metres)."""
        code = {"cross": _lib.TT_RENDER_MARKER_CROSS, "box": _lib.TT_RENDER_MARKER_BOX}[shape]
        x, y, w, h = clip if clip is not None else (0, 0, self.width, self.height)
        return self._add(_lib.TT_RENDER_MARKER, x, y, w, h, count=code, color=_color(color), alpha=int(alpha), half_width=int(half_width),
                         radius=int(radius), m=np.asarray(matrix, np.float32).reshape(6),
                         p=[center[0], center[1], half[0], half[1]])

    def text(self, string, x, y, color=(255, 255, 255), scale=1, alpha=256):
        data = string if isinstance(string, (bytes, bytearray)) else str(string).encode("latin-1", "replace")
        if bytes(data) not in self._text_at:
            self._text_at[bytes(data)] = len(self.text_bytes)
            self.text_bytes += data
        font = self.side["font"]
        self._add(_lib.TT_RENDER_TEXT, x, y, 6 * len(data) * scale, 8 * scale, (font,), count=len(data), scale=int(scale),
                  channels=NUM_GLYPHS, color=_color(color), alpha=int(alpha), aux=font.data_ptr())
        self.refs[-1] += (("text", self._text_at[bytes(data)], bytes(data)),)
        return self

    def bar(self, x, y, w, h, value, lo=0.0, hi=1.0, color=(255, 255, 255), back=(48, 48, 48)):
        """A horizontal gauge of a HOST number: the background, then the part from the zero of [lo, hi] to `value`."""
        self.fill(x, y, w, h, back)
        v = min(max(float(value), lo), hi) if np.isfinite(value) else lo
        zero = min(max(0.0, lo), hi)
        a, b = sorted((int(round((zero - lo) / (hi - lo) * w)), int(round((v - lo) / (hi - lo) * w))))
        return self.fill(x + a, y + 1, b - a, h - 2, color)

    # -------------------------------------------------------------------------------------------------------------- the table
    def packed_bytes(self):
        return _up(ITEM_BYTES * len(self.items) + len(self.text_bytes), 16)

    def pack(self, base):
        """-> (the ctypes table with every text run's pointer resolved, the bytes to place at address `base`: the table and the
        text pool behind it).  A table of no items is one zeroed item long."""
        n = len(self.items)
        table = (Item * max(n, 1))()
        for i, (it, refs) in enumerate(zip(self.items, self.refs)):
            ctypes.memmove(ctypes.byref(table[i]), ctypes.byref(it), ITEM_BYTES)
            if it.kind == _lib.TT_RENDER_TEXT:
                table[i].src = base + ITEM_BYTES * n + refs[-1][1]
        raw = bytes(table)[:ITEM_BYTES * n] + bytes(self.text_bytes)
        return table, raw + bytes(self.packed_bytes() - len(raw))

    def workspace_bytes(self):
        return self._plane_at


class Rasteriser:
    """Owns the device side of drawing on one device: the table buffer and the workspace (zeroed when it is allocated; the entry
    leaves the planes zeroed).  All calls of one Rasteriser must be on ONE stream."""

    def __init__(self, device="cuda"):
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("Rasteriser needs a GPU device: there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._table = self._work = None

    def draw(self, dl, out=None):
        """-> uint8 (height, width, 3) on the device, queued on the current stream; nothing waits."""
        import torch
        from .ops import check, lib, ptr
        n = len(dl)
        if n > _lib.TT_RENDER_MAX_ITEMS:
            raise ValueError(f"{n} items in one list, at most {_lib.TT_RENDER_MAX_ITEMS}")
        if out is None:
            out = torch.empty(dl.height, dl.width, 3, dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (dl.height, dl.width, 3) or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out: contiguous uint8 ({dl.height}, {dl.width}, 3) on {self.device} is needed")
        need = dl.packed_bytes()
        if self._table is None or self._table.numel() < need:
            self._table = torch.empty(_up(max(need, 1), 1 << 14), dtype=torch.uint8, device=self.device)
        if self._work is None or self._work.numel() < dl.workspace_bytes():
            self._work = torch.zeros(_up(dl.workspace_bytes(), 1 << 16), dtype=torch.uint8, device=self.device)
        table, raw = dl.pack(self._table.data_ptr())
        with torch.cuda.device(self.device):
            if raw:
                self._table[:len(raw)].copy_(torch.from_numpy(np.frombuffer(raw, np.uint8).copy()), non_blocking=False)
            check(lib().tt_render_u8(ptr(out), dl.height, dl.width, table, ptr(self._table), n, ptr(self._work), self._work.numel(),
                                     torch.cuda.current_stream(self.device).cuda_stream), "tt_render_u8")
        self._keep = (dl, table)                             # (the kernels read the list's tensors after this returns)
        return out

    def status(self, reset=True):
        """The status words (TT_RENDER_STATUS_DROPPED: polyline and marker points dropped since the last reset).  WAITS for the device."""
        import torch
        if self._work is None:
            return [0] * _lib.TT_RENDER_STATUS_WORDS
        words = self._work[:8 * _lib.TT_RENDER_STATUS_WORDS].view(torch.int64)
        out = words.cpu().tolist()
        if reset:
            words.zero_()
        return out


# ------------------------------------------------------------------------------------------------------------ the composed view
def bev_matrices(panel, x_bound, y_bound):
    """The 2 x 3 matrices from metres to 1/16 px of the canvas for everything drawn in the BEV panel `panel` = (x, y, w, h), forward
    UP -- the one place where the conventions meet:
      cloud      rows (x forward, y right, z up): the simulator's LiDAR frame, as the agent hands it on;
      waypoints  pred_wp[..., 0] forward, [..., 1] to the right: control_pid reverses the pair before arctan2(forward, right);
      target     the same pair in the same order: control_pid reverses it with the waypoints.
    So the three are ONE matrix: u = ox + s * right, v = oy - s * forward, with s the panel's scale in 1/16 px per metre (an integer,
    so every entry is exact in f32) and (ox, oy) the ego origin: x_bound's upper end at the panel's top, y_bound centred.
    -> {"cloud", "waypoints", "target": (2, 3) float32, "scale16": s, "origin16": (ox, oy)}"""
    px, py, pw, ph = panel
    scale16 = int(min(16 * pw / (y_bound[1] - y_bound[0]), 16 * ph / (x_bound[1] - x_bound[0])))
    ox = 16 * px + int(round(-y_bound[0] * scale16))
    oy = 16 * py + int(round(x_bound[1] * scale16))
    m = np.array([[0.0, scale16, ox], [-scale16, 0.0, oy]], np.float32)
    return {"cloud": m, "waypoints": m.copy(), "target": m.copy(), "scale16": scale16, "origin16": (ox, oy)}


def default_layout(final_dim, num_cams=4):
    """{panel: (x, y, w, h)} for network inputs of final_dim = (fh, fw): the cameras 2 x 2, each with its depth map (fh / 2 x fw / 2,
    i.e. the fh / 16 map at k = 8) to its right; the square BEV panel beside them; the HUD strip underneath."""
    fh, fw = int(final_dim[0]), int(final_dim[1])
    cell = fw + fw // 2
    lay = {}
    for n in range(num_cams):
        cx, cy = (n % 2) * cell, (n // 2) * fh
        lay[f"cam{n}"] = (cx, cy, fw, fh)
        lay[f"depth{n}"] = (cx + fw, cy, fw // 2, fh // 2)
    rows = (num_cams + 1) // 2
    side = rows * fh
    lay["bev"] = (2 * cell, 0, side, side)
    lay["hud"] = (0, side, 2 * cell + side, 40)
    lay["canvas"] = (0, 0, 2 * cell + side, side + 40)
    return lay


EGO_HALF = (2.45, 1.05)                  # half length (forward) and half width of the ego box, metres


class DebugRenderer:
    """The composed debug view of one sample: see `default_layout`.  `frame` queues one tt_render_u8 on the current stream and
    returns the canvas; nothing crosses to the host (the HUD's numbers are host numbers already)."""

    def __init__(self, model_cfg=None, layout=None, device="cuda"):
        from . import config
        cfg = model_cfg if model_cfg is not None else config.model_config()
        enc = cfg["img_encoder"]
        self.final_dim = tuple(enc["final_dim"])
        self.num_cams = int(cfg.get("num_cams", 4))
        self.x_bound, self.y_bound = tuple(enc["x_bound"][:2]), tuple(enc["y_bound"][:2])
        self.depth_bins = int(round((enc["d_bound"][1] - enc["d_bound"][0]) / enc["d_bound"][2]))
        self.depth_factor = int(enc["downsample_factor"])
        self.num_classes = int(enc["seg_net_conf"]["out_channels"])
        self.layout = dict(layout) if layout is not None else default_layout(self.final_dim, self.num_cams)
        self.matrices = bev_matrices(self.layout["bev"], self.x_bound, self.y_bound)
        self.raster = Rasteriser(device)
        self.device = self.raster.device

    def display_list(self, img, pred, cloud, b=0, controls=None, target=None, gt_wp=None):
        """The frame as a DisplayList (what `frame` draws)."""
        lay, M = self.layout, self.matrices
        _, _, W, H = lay["canvas"]
        dl = DisplayList(H, W, self.device)
        N = self.num_cams
        if img.dim() == 6:                                   # a batch's (B, T, N, 3, h, w): the key sweep is the last
            img = img[b, -1]
        elif img.dim() == 5:
            img = img[b]
        fh, fw = img.shape[-2], img.shape[-1]
        seg = pred.get("_seg_cl") if pred is not None else None
        dep = pred.get("_depth_cl") if pred is not None else None
        for n in range(N):
            x, y, w, h = lay[f"cam{n}"]
            dl.image(img[n], x, y, w=min(w, fw), h=min(h, fh))
            if seg is not None:
                s = seg[b * N + n]
                f = fh // s.shape[0]
                dl.seg_overlay(s, x, y, factor=f, num_classes=self.num_classes, w=min(w, s.shape[1] * f), h=min(h, s.shape[0] * f))
            x, y, w, h = lay[f"depth{n}"]
            dl.fill(x, y, w, h, (16, 16, 16))
            if dep is not None:
                d = dep[b * N + n]
                k = max(1, self.depth_factor // 2)
                dl.depth_map(d, x, y, scale=k, bins=self.depth_bins, w=min(w, d.shape[1] * k), h=min(h, d.shape[0] * k))
        bev = lay["bev"]
        dl.fill(*bev, (10, 10, 24))
        if cloud is not None:
            dl.points_bev(cloud, *bev, M["cloud"])
        dl.marker("box", (0.0, 0.0), EGO_HALF, M["waypoints"], (255, 255, 255), half_width=12, clip=bev)
        if gt_wp is not None:
            dl.polyline(gt_wp[b] if gt_wp.dim() == 3 else gt_wp, M["waypoints"], (255, 255, 255), half_width=20, radius=44, clip=bev)
        if pred is not None and pred.get("pred_wp") is not None:
            wp = pred["pred_wp"]
            S = wp.shape[1]
            for s in range(S):
                last = s == S - 1
                dl.polyline(wp[b, s], M["waypoints"], STAGE_COLORS[(len(STAGE_COLORS) - S + s) % len(STAGE_COLORS)],
                            half_width=28 if last else 12, radius=56 if last else 32, clip=bev)
        if target is not None:
            dl.marker("cross", (float(target[0]), float(target[1])), (1.0, 1.0), M["target"], (255, 64, 64), half_width=16, clip=bev)
        self._hud(dl, lay["hud"], controls or {})
        return dl

    @staticmethod
    def _num(v, fmt="%+.2f"):
        try:
            v = float(v)
        except (TypeError, ValueError):
            return "-"
        return fmt % v if np.isfinite(v) else "NAN"

    def _hud(self, dl, hud, c):
        x, y, w, h = hud
        dl.fill(x, y, w, h, (0, 0, 0))
        col = max(120, min(w // 5, 300))
        gauges = (("STEER", "steer", -1.0, 1.0, (90, 170, 255)), ("THR", "throttle", 0.0, 1.0, (90, 230, 90)), ("BRK", "brake", 0.0, 1.0, (255, 80, 80)))
        for i, (label, key, lo, hi, color) in enumerate(gauges):
            gx = x + 4 + i * col
            dl.text(f"{label} {self._num(c.get(key))}", gx, y + 3)
            dl.bar(gx, y + 14, col - 12, 8, c.get(key, 0.0) if isinstance(c.get(key), (int, float)) else 0.0, lo, hi, color)
            if f"{key}_ctrl" in c or f"{key}_traj" in c:
                dl.text(f"C{self._num(c.get(key + '_ctrl'))} T{self._num(c.get(key + '_traj'))}", gx, y + 26, (180, 180, 180))
        gx = x + 4 + 3 * col
        dl.text(f"SPEED {self._num(c.get('speed'), '%.2f')} M/S", gx, y + 3)
        if "step" in c:
            dl.text(f"STEP {int(c['step'])}", gx, y + 14)
        if c.get("is_stuck"):
            dl.text("STUCK", gx, y + 26, (255, 80, 80))

    def frame(self, img, pred, cloud, b=0, controls=None, target=None, gt_wp=None):
        """img: the network input (N, 3, h, w) or a batch's (B, T, N, 3, h, w); pred: forward_inference's dict, or None (cameras and
        cloud only); cloud: (n, >= 3) f32 or None; controls: host numbers for the HUD (steer, throttle, brake, speed, step and the
        *_ctrl / *_traj values); target: the (forward, right) target point, host; gt_wp: (4, 2) or (B, 4, 2) device waypoints, drawn
        in white under the predictions.  -> uint8 (Hc, Wc, 3) device tensor, queued on the current stream."""
        return self.raster.draw(self.display_list(img, pred, cloud, b, controls, target, gt_wp))

    def status(self, reset=True):
        return self.raster.status(reset)
