"""thinktwice_amd.render without a GPU: the packed table against the header's struct, the font, the palette, the default layout,
the BEV matrices, the entry's refusals (which come before any launch) and AgentTick's argument check."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import render_cases as R  # noqa: E402
from thinktwice_amd import _lib, config, render  # noqa: E402

Item = _lib.structs()["tt_render_item"]


def test_display_list_packs_what_the_headers_struct_says():
    assert ctypes.sizeof(Item) == render.ITEM_BYTES == 128
    want = dict(kind=(0, "i"), x0=(4, "i"), y0=(8, "i"), w=(12, "i"), h=(16, "i"), sw=(20, "i"), sh=(24, "i"), scale=(28, "i"),
                channels=(32, "i"), stride=(36, "i"), count=(40, "i"), alpha=(44, "i"), color=(48, "I"), half_width=(52, "i"),
                radius=(56, "i"), reserved=(60, "i"), m=(64, "6f"), p=(88, "4f"), ws_offset=(104, "q"), src=(112, "Q"), aux=(120, "Q"))
    assert [n for n, _ in Item._fields_] == list(want)
    for name, (offset, fmt) in want.items():
        assert getattr(Item, name).offset == offset and getattr(Item, name).size == struct.calcsize("<" + fmt), name
    arena = R.Arena("cpu", 1 << 16)
    dl = render.DisplayList(33, 65, "cpu", side=arena.side())
    seg = arena.put(np.zeros((4, 6, 16), np.float32))
    cloud = arena.put(np.ones((7, 5), np.float32))
    dl.fill(1, 2, 3, 4, (5, 6, 7), alpha=99).seg_overlay(seg, -3, 9, factor=2).text("AB", 4, 5, (1, 2, 3), scale=3)
    dl.points_bev(cloud, 8, 9, 10, 11, [[1, 2, 3], [4, 5, 6]], z_lo=-1.0, z_hi=7.0).points_bev(cloud, 0, 0, 10, 20, R.IDENT16)
    dl.polyline(cloud[:3, :2], R.IDENT16, (255, 0, 0), half_width=9, radius=21, clip=(1, 1, 30, 30))
    base = 0x7000
    table, raw = dl.pack(base)
    assert len(raw) == dl.packed_bytes() and len(raw) % 16 == 0 and raw[128 * 6:128 * 6 + 2] == b"AB"

    def field(i, name):
        v = struct.unpack_from("<" + want[name][1], raw, 128 * i + want[name][0])
        return v[0] if len(v) == 1 else list(v)
    assert [field(0, k) for k in ("kind", "x0", "y0", "w", "h", "alpha", "color")] == [_lib.TT_RENDER_FILL, 1, 2, 3, 4, 99, 5 | 6 << 8 | 7 << 16]
    assert [field(1, k) for k in ("kind", "x0", "y0", "w", "h", "sw", "sh", "scale", "channels", "stride")] == \
        [_lib.TT_RENDER_SEG_OVERLAY, -3, 9, 12, 8, 6, 4, 2, 12, 16]
    assert field(1, "src") == seg.data_ptr() and field(1, "aux") == dl.side["palette"].data_ptr()
    assert [field(2, k) for k in ("kind", "w", "h", "count", "scale", "channels")] == [_lib.TT_RENDER_TEXT, 36, 24, 2, 3, render.NUM_GLYPHS]
    assert field(2, "src") == base + 128 * 6 and field(2, "aux") == dl.side["font"].data_ptr()
    assert [field(3, k) for k in ("kind", "count", "stride", "ws_offset", "m")] == [_lib.TT_RENDER_POINTS_BEV, 7, 5, 256, [1, 2, 3, 4, 5, 6]]
    assert field(3, "p")[:2] == [-1.0, 32.0] and field(4, "ws_offset") == 256 + 512 and dl.workspace_bytes() == 256 + 512 + 1024
    assert [field(5, k) for k in ("kind", "count", "half_width", "radius", "x0", "y0", "w", "h")] == [_lib.TT_RENDER_POLYLINE_DEV, 3, 9, 21, 1, 1, 30, 30]
    assert bytes(table)[:128 * 6] == raw[:128 * 6]


def test_glyphs_are_pairwise_distinct_and_non_empty_except_space():
    need = set("0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ.-+:%/ ")
    assert need <= set(render.GLYPH_CHARS)
    rows = {ch: tuple(render.glyph_rows(ch)) for ch in render.GLYPH_CHARS}
    rows["unknown"] = tuple(render.glyph_rows("~"))
    assert len(set(rows.values())) == len(rows)
    for ch, r in rows.items():
        assert len(r) == 7 and all(0 <= v < 32 for v in r)
        assert (sum(r) == 0) == (ch == " "), ch
    table = render.font_table()
    assert len(table) == 256 + 8 * render.NUM_GLYPHS and table[:256].max() == render.NUM_GLYPHS - 1
    for ch in render.GLYPH_CHARS:
        g = int(table[ord(ch)])
        assert tuple(table[256 + 8 * g:256 + 8 * g + 7]) == rows[ch] and table[ord(ch.lower())] == g
    assert table[ord("~")] == 0 and tuple(table[256:263]) == rows["unknown"]


def test_palette_has_one_entry_per_class_and_only_the_background_is_transparent():
    C = config.model_config()["img_encoder"]["seg_net_conf"]["out_channels"]
    pal = render.seg_palette(C)
    assert pal.shape == (C, 4) and pal.dtype == np.uint8
    assert pal[0, 3] == 0 and (pal[1:, 3] > 0).all()
    assert len({tuple(p[:3]) for p in pal[1:]}) == C - 1
    for lut in (render.depth_lut(), render.height_lut()):
        assert lut.shape == (256, 3) and lut.dtype == np.uint8 and not (lut == np.array(render.NONFINITE)).all(1).any()


@pytest.mark.parametrize("final_dim", [(448, 896), (128, 256)])
def test_default_layout_panels_do_not_overlap_and_lie_inside_the_canvas(final_dim):
    lay = render.default_layout(final_dim)
    _, _, W, H = lay["canvas"]
    panels = {k: v for k, v in lay.items() if k != "canvas"}
    assert set(panels) == {f"cam{n}" for n in range(4)} | {f"depth{n}" for n in range(4)} | {"bev", "hud"}
    for k, (x, y, w, h) in panels.items():
        assert w > 0 and h > 0 and x >= 0 and y >= 0 and x + w <= W and y + h <= H, k
    names = sorted(panels)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            (ax, ay, aw, ah), (bx, by, bw, bh) = panels[a], panels[b]
            assert ax + aw <= bx or bx + bw <= ax or ay + ah <= by or by + bh <= ay, (a, b)
    for n in range(4):
        assert panels[f"cam{n}"][2:] == (final_dim[1], final_dim[0]) and panels[f"depth{n}"][2:] == (final_dim[1] // 2, final_dim[0] // 2)


def test_bev_matrices_put_the_ego_at_its_box_and_forward_up():
    cfg = config.model_config()["img_encoder"]
    panel = render.default_layout((448, 896))["bev"]
    M = render.bev_matrices(panel, cfg["x_bound"], cfg["y_bound"])
    s, (ox, oy) = M["scale16"], M["origin16"]
    px, py, pw, ph = panel
    assert isinstance(s, int) and s == int(16 * pw / 38.4) and 16 * px < ox < 16 * (px + pw) and 16 * py < oy < 16 * (py + ph)
    assert abs(ox - 16 * (px + pw / 2)) <= 16 and abs(oy - (16 * py + 30.4 * s)) <= 1            # y centred, x_bound's top at the top
    for key in ("waypoints", "target", "cloud"):
        m = M[key].astype(np.float64)
        assert M[key].dtype == np.float32 and m.shape == (2, 3)
        at = lambda fwd, right: (m[0, 0] * fwd + m[0, 1] * right + m[0, 2], m[1, 0] * fwd + m[1, 1] * right + m[1, 2])   # noqa: E731
        assert at(0, 0) == (ox, oy)                              # the centre of the ego box, a MARKER centred on (0, 0)
        assert at(10, 0) == (ox, oy - 10 * s)                    # 10 m ahead: straight up by 10 s / 16 pixels
        assert at(0, 3) == (ox + 3 * s, oy)                      # 3 m to the right: to the right
    assert render.EGO_HALF[0] > render.EGO_HALF[1] > 0           # the composed view draws the ego box about (0, 0), longer than wide


def test_workspace_bytes_agree_and_refusals_come_before_any_launch():
    lib = _lib.lib()
    for c in R.cases("cpu"):
        table, start, _ = R.place_table(c)
        n = len(c.dl)
        fake = 0x10000                                           # (never dereferenced: a refusal comes first)
        if c.expect_error:
            rc = lib.tt_render_u8(fake, c.dl.height, c.dl.width, table, c.arena.blob.data_ptr() + start, n, fake, 1 << 30, None)
            assert rc != 0 and b"tt_render_u8" in lib.tt_last_error(), c.name
        elif n:
            assert lib.tt_render_workspace_bytes(table, n) == c.dl.workspace_bytes(), c.name
    good = next(c for c in R.cases("cpu") if c.name.startswith("clouds"))
    table, start, _ = R.place_table(good)
    dev, n, ws = good.arena.blob.data_ptr() + start, len(good.dl), good.dl.workspace_bytes()
    for canvas, Hc, Wc, tab, at, cnt, work, size in ((None, 40, 72, table, dev, n, 0x10000, ws), (0x10000, 40, 72, None, dev, n, 0x10000, ws), (0x10000, 40, 72, table, None, n, 0x10000, ws),
                 (0x10000, 40, 72, table, dev, n, None, ws), (0x10000, 40, 72, table, dev, n, 0x10000, ws - 1), (0x10000, 0, 72, table, dev, n, 0x10000, ws),
                 (0x10000, 40, 16385, table, dev, n, 0x10000, ws), (0x10000, 40, 72, table, dev + 8, n, 0x10000, ws),
                 (0x10000, 40, 72, table, dev, n, 0x10010, ws), (0x10000, 40, 72, table, dev, -1, 0x10000, ws)):
        assert lib.tt_render_u8(canvas, Hc, Wc, tab, at, cnt, work, size, None) != 0, (canvas, Hc, Wc, at, cnt, work, size)
    assert lib.tt_render_workspace_bytes(None, 3) == 0 and lib.tt_render_workspace_bytes(table, _lib.TT_RENDER_MAX_ITEMS + 1) == 0
    assert lib.tt_render_workspace_bytes(None, 0) == 256


def test_agent_tick_with_render_needs_a_recorder():
    from thinktwice_amd.agent_tick import AgentTick
    with pytest.raises(ValueError, match="recorder"):
        AgentTick(None, render=True, recorder=None)
