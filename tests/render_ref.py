"""numpy restatement of tt_render_u8 (include/thinktwice_hip.h), structured the other way round from the kernel: it loops over the
ITEMS and paints each one over the whole canvas with array operations (the kernel loops over pixels and walks the items), so the
two fail differently.  f32 arithmetic is numpy float32, one rounding per operation; integers are int64, and Python integers where
a product passes 64 bits.  `render(dl)` takes a render.DisplayList (its tensors on any device) -> (canvas uint8 (H, W, 3), the
number of dropped polyline / marker points)."""
import numpy as np

from thinktwice_amd import _lib
from thinktwice_amd import render as tt_render

F = np.float32
LIMIT = F(1 << 20)


def _np(t):
    return t.detach().cpu().numpy()


def _rgb(color):
    return np.array([color & 255, color >> 8 & 255, color >> 16 & 255], np.int64)


def _blend(canvas, box, src, weight, mask=None):
    """canvas[box] = (dst * (256 - a) + src * a + 128) >> 8 where mask; src (h, w, 3) or (3,), weight (h, w) or a number."""
    y0, y1, x0, x1 = box
    dst = canvas[y0:y1, x0:x1].astype(np.int64)
    a = np.broadcast_to(np.asarray(weight, np.int64), dst.shape[:2])[..., None]
    out = (dst * (256 - a) + np.broadcast_to(src, dst.shape) * a + 128) >> 8
    if mask is not None:
        out = np.where(mask[..., None], out, dst)
    canvas[y0:y1, x0:x1] = out.astype(np.uint8)


def _clip(it, H, W):
    x0, y0, x1, y1 = max(it.x0, 0), max(it.y0, 0), min(it.x0 + it.w, W), min(it.y0 + it.h, H)
    return None if x0 >= x1 or y0 >= y1 else (y0, y1, x0, x1)


def _window(full, it, box):
    """The part of an item-sized array (its [0, 0] at the item's corner) that lies under the clipped box."""
    y0, y1, x0, x1 = box
    return full[y0 - it.y0:y1 - it.y0, x0 - it.x0:x1 - it.x0]


def _affine(m, x, y):
    x, y = np.asarray(x, F), np.asarray(y, F)
    with np.errstate(all="ignore"):
        u = (F(m[0]) * x + F(m[1]) * y) + F(m[2])
        v = (F(m[3]) * x + F(m[4]) * y) + F(m[5])
    return u, v


def _logit_classes(t, it):
    """(sh, sw) argmax over the first `channels` logits, ties to the lowest; -1 where a cell holds a NaN."""
    z = _np(t)[:, :, :it.channels]
    return np.where(np.isnan(z).any(-1), -1, np.argmax(np.where(np.isnan(z), -np.inf, z), -1))


def _upscaled(cells, k, it):
    return np.repeat(np.repeat(cells, k, 0), k, 1)[:it.h, :it.w]


def poly_points(it, refs):
    """-> (fixed-point xs, ys as Python-int lists, the valid flags, the segments as index pairs, the dropped count)."""
    if it.kind == _lib.TT_RENDER_POLYLINE_DEV:
        pts = _np(refs[0]).reshape(-1, 2).astype(F) if it.count else np.zeros((0, 2), F)
        x, y = pts[:, 0], pts[:, 1]
        pairs = [(i, i + 1) for i in range(len(x) - 1)]
    else:
        cx, cy, hx, hy = (F(v) for v in it.p)
        with np.errstate(over="ignore"):                         # (a sum may overflow to inf, as on the device: the point is dropped)
            if it.count == _lib.TT_RENDER_MARKER_BOX:
                x, y = np.array([cx - hx, cx + hx, cx + hx, cx - hx], F), np.array([cy - hy, cy - hy, cy + hy, cy + hy], F)
                pairs = [(0, 1), (1, 2), (2, 3), (3, 0)]
            else:
                x, y = np.array([cx - hx, cx + hx, cx, cx], F), np.array([cy, cy, cy - hy, cy + hy], F)
                pairs = [(0, 1), (2, 3)]
    u, v = _affine(it.m, x, y)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(x) & np.isfinite(y) & (np.abs(u) <= LIMIT) & (np.abs(v) <= LIMIT)
    fx = [int(np.rint(a)) if o else None for a, o in zip(u, ok)]
    fy = [int(np.rint(a)) if o else None for a, o in zip(v, ok)]
    return fx, fy, list(ok), pairs, int((~ok).sum())


def _cover(mask, box, cx0, cy0, inside):
    """OR `inside(cx, cy)` (pixel centres in 1/16 px, object arrays of Python ints) into mask over the pixel box cut to `box`."""
    y0, y1, x0, x1 = box
    bx0, bx1, by0, by1 = max(cx0[0], x0), min(cx0[1], x1), max(cy0[0], y0), min(cy0[1], y1)
    if bx0 >= bx1 or by0 >= by1:
        return
    cx = (16 * np.arange(bx0, bx1, dtype=np.int64) + 8).astype(object)[None, :]
    cy = (16 * np.arange(by0, by1, dtype=np.int64) + 8).astype(object)[:, None]
    mask[by0 - y0:by1 - y0, bx0 - x0:bx1 - x0] |= np.asarray(inside(cx, cy), bool)


def _poly_mask(it, refs, box):
    fx, fy, ok, pairs, dropped = poly_points(it, refs)
    y0, y1, x0, x1 = box
    mask = np.zeros((y1 - y0, x1 - x0), bool)
    r2, hw2 = it.radius ** 2, it.half_width ** 2

    def reach(lo, hi, r):                                    # pixels whose centre can lie within r of [lo, hi]
        return ((lo - r - 8) // 16, (hi + r - 8) // 16 + 1)
    if it.radius > 0:
        for x, y, o in zip(fx, fy, ok):
            if o:
                _cover(mask, box, reach(x, x, it.radius), reach(y, y, it.radius), lambda cx, cy: (cx - x) ** 2 + (cy - y) ** 2 <= r2)
    for a, b in pairs:
        if not (ok[a] and ok[b]):
            continue
        ax, ay, bx, by = fx[a], fy[a], fx[b], fy[b]
        dx, dy = bx - ax, by - ay
        len2 = dx * dx + dy * dy

        def inside(cx, cy):
            qx, qy = cx - ax, cy - ay
            t = qx * dx + qy * dy
            before = (t <= 0) & (qx * qx + qy * qy <= hw2)
            after = (t >= len2) & ((cx - bx) ** 2 + (cy - by) ** 2 <= hw2)
            cross = qx * dy - qy * dx
            between = (t > 0) & (t < len2) & (cross * cross <= hw2 * len2)
            return (before | after | between).astype(bool)
        _cover(mask, box, reach(min(ax, bx), max(ax, bx), it.half_width), reach(min(ay, by), max(ay, by), it.half_width), inside)
    return mask, dropped


def render(dl):
    H, W = dl.height, dl.width
    canvas = np.zeros((H, W, 3), np.uint8)
    dropped = 0
    for it, refs in zip(dl.items, dl.refs):
        box = _clip(it, H, W)
        kind = it.kind
        if kind in (_lib.TT_RENDER_POLYLINE_DEV, _lib.TT_RENDER_MARKER):
            if box is None:
                dropped += poly_points(it, refs)[4]
                continue
            mask, d = _poly_mask(it, refs, box)
            dropped += d
            _blend(canvas, box, _rgb(it.color), it.alpha, mask)
            continue
        if box is None:
            continue
        if kind == _lib.TT_RENDER_FILL:
            _blend(canvas, box, _rgb(it.color), it.alpha)
        elif kind == _lib.TT_RENDER_IMAGE_F32:
            src = _np(refs[0]).astype(F)
            nan = np.isnan(src).any(0)
            with np.errstate(all="ignore"):
                q = np.stack([np.rint(src[c] * F(it.m[c]) + F(it.m[3 + c])) for c in range(3)], -1)
            q = np.clip(np.where(np.isnan(q), F(0), q), 0, 255).astype(np.int64)
            q = np.where(nan[..., None], _rgb(it.color), q)
            _blend(canvas, box, _window(_upscaled(q, it.scale, it), it, box), it.alpha)
        elif kind == _lib.TT_RENDER_IMAGE_U8:
            src = _np(refs[0]).reshape(it.sh, it.sw, it.channels).astype(np.int64)
            s, gh, gw = it.scale, it.sh // it.scale, it.sw // it.scale
            small = (src[:gh * s, :gw * s].reshape(gh, s, gw, s, it.channels).sum((1, 3)) + s * s // 2) // (s * s)
            small = np.broadcast_to(small, (gh, gw, 3)) if it.channels == 1 else small
            _blend(canvas, box, _window(small[:it.h, :it.w], it, box), it.alpha)
        elif kind in (_lib.TT_RENDER_SEG_OVERLAY, _lib.TT_RENDER_DEPTH_MAP):
            cls = _window(_upscaled(_logit_classes(refs[0], it), it.scale, it), it, box)
            table = _np(refs[1]).astype(np.int64)
            if kind == _lib.TT_RENDER_SEG_OVERLAY:
                pal = table[:4 * it.channels].reshape(-1, 4)
                colour, weight = pal[np.maximum(cls, 0), :3], pal[np.maximum(cls, 0), 3]
                weight = weight + (weight >> 7)
            else:
                index = np.maximum(cls, 0) * 255 // (it.channels - 1) if it.channels > 1 else np.zeros_like(cls)
                colour, weight = table[:768].reshape(256, 3)[index], np.full(cls.shape, it.alpha)
            colour = np.where((cls < 0)[..., None], _rgb(it.color), colour)
            _blend(canvas, box, colour, np.where(cls < 0, 256, weight))
        elif kind == _lib.TT_RENDER_POINTS_BEV:
            plane = np.zeros((it.h, it.w), np.int64)
            if it.count:
                pts = _np(refs[0]).astype(F)
                x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
                u, v = _affine(it.m, x, y)
                with np.errstate(all="ignore"):
                    u, v = np.floor(u), np.floor(v)
                    keep = ~((x == 0) & (y == 0) & (z == 0)) & np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
                    keep &= (np.abs(u) <= LIMIT) & (np.abs(v) <= LIMIT)
                    height = np.floor((z - F(it.p[0])) * F(it.p[1]))
                px = np.where(keep, u, 0).astype(np.int64) >> 4
                py = np.where(keep, v, 0).astype(np.int64) >> 4
                keep &= (px >= max(it.x0, 0)) & (px < min(it.x0 + it.w, W)) & (py >= max(it.y0, 0)) & (py < min(it.y0 + it.h, H))
                idx = np.clip(np.where(np.isnan(height), F(0), height), 0, 255).astype(np.int64)
                np.maximum.at(plane, (py[keep] - it.y0, px[keep] - it.x0), idx[keep] + 1)
            hit = _window(plane, it, box)
            lut = _np(refs[1]).astype(np.int64)[:768].reshape(256, 3)
            _blend(canvas, box, lut[np.maximum(hit - 1, 0)], it.alpha, hit > 0)
        elif kind == _lib.TT_RENDER_TEXT:
            data = refs[-1][2]
            bitmap = np.zeros((8, 6 * len(data)), bool)
            for i, ch in enumerate(data):
                rows = tt_render.glyph_rows(chr(ch))
                for r, bits in enumerate(rows):
                    bitmap[r, 6 * i:6 * i + 5] = [(bits >> (4 - c)) & 1 for c in range(5)]
            big = np.kron(bitmap, np.ones((it.scale, it.scale), bool))[:it.h, :it.w]
            _blend(canvas, box, _rgb(it.color), it.alpha, _window(big, it, box))
        else:
            raise ValueError(f"unknown kind {kind}")
    return canvas, dropped
