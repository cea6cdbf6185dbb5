"""tt_render_u8 on the GPU against the numpy restatement (tests/render_ref.py), over the display lists of tests/render_cases.py:
every canvas and dropped-point count to the byte, the guard bytes around the canvas and behind the workspace untouched, the
workspace's planes zero again after every call, two runs identical, refusals without a write; and render.DebugRenderer's default
frame of a synthetic batch at the test model size against the restatement fed the same tensors."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import render_cases as R  # noqa: E402
import render_ref  # noqa: E402
from thinktwice_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, STATUS = R.GUARD, 8 * _lib.TT_RENDER_STATUS_WORDS
NAMES = [c.name for c in R.cases("cpu")]                    # (the names only: the device's cases are built when a test runs)
GOOD = [c.name for c in R.cases("cpu") if not c.expect_error]


def _case(name):
    return next(c for c in R.cases("cuda") if c.name == name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    return render_ref.render(_case(name).dl)


def _draw(case, work=None):
    """One tt_render_u8 -> (rc, the canvas buffer with its guards, the workspace with its guard, its bytes)."""
    from thinktwice_amd.ops import lib
    table, start, _ = R.place_table(case)
    H, W, n = case.dl.height, case.dl.width, len(case.dl)
    buf = torch.full((2 * GUARD + H * W * 3,), 0xA5, dtype=torch.uint8, device="cuda")
    ws_bytes = case.dl.workspace_bytes() if not case.expect_error else 1 << 16
    if work is None:
        work = torch.zeros(ws_bytes + GUARD, dtype=torch.uint8, device="cuda")
        work[ws_bytes:] = 0xA5
    rc = lib().tt_render_u8(buf.data_ptr() + GUARD, H, W, table, case.arena.blob.data_ptr() + start, n, work.data_ptr(), ws_bytes,
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, buf, work, ws_bytes


def _parts(case, buf):
    H, W = case.dl.height, case.dl.width
    b = buf.cpu().numpy()
    return b[:GUARD], b[GUARD:GUARD + H * W * 3].reshape(H, W, 3), b[GUARD + H * W * 3:]


@pytest.mark.parametrize("name", GOOD)
def test_canvas_counters_guards_and_workspace(name):
    case = _case(name)
    want, dropped = _reference(name)
    rc, buf, work, ws_bytes = _draw(case)
    assert rc == 0
    before, canvas, after = _parts(case, buf)
    w = work.cpu().numpy()
    print(f"{name}: {int((canvas != want).any(-1).sum())} pixels differ, dropped {int(w[:8].view(np.int64)[0])} / {dropped}")
    assert np.array_equal(canvas, want)
    assert int(w[:8].view(np.int64)[0]) == dropped and not w[8:STATUS].any()
    assert (before == 0xA5).all() and (after == 0xA5).all() and (w[ws_bytes:] == 0xA5).all()
    assert not w[STATUS:ws_bytes].any()                      # the planes are zero again
    rc, buf2, _, _ = _draw(case, work)                       # the same workspace again: the same picture, the counter added to
    assert rc == 0 and torch.equal(buf, buf2)
    w = work.cpu().numpy()
    assert int(w[:8].view(np.int64)[0]) == 2 * dropped and not w[STATUS:ws_bytes].any()


def test_a_second_list_on_the_same_workspace_gives_its_own_picture():
    a, b = _case("clouds_40x72"), _case("clouds_33x65")
    size = max(a.dl.workspace_bytes(), b.dl.workspace_bytes())
    work = torch.zeros(size + GUARD, dtype=torch.uint8, device="cuda")
    for case in (a, b, a):
        rc, buf, _, _ = _draw(case, work)
        assert rc == 0 and np.array_equal(_parts(case, buf)[1], _reference(case.name)[0]), case.name
        assert not work[STATUS:].any()


@pytest.mark.parametrize("name", [n for n in NAMES if n not in GOOD])
def test_refused_lists_write_nothing(name):
    from thinktwice_amd.ops import lib
    rc, buf, work, _ = _draw(_case(name))
    assert rc != 0 and b"tt_render_u8" in lib().tt_last_error()
    assert (buf == 0xA5).all() and not work[:1 << 16].any()


def test_reversed_segments_cover_the_same_pixels_on_the_device():
    for hw in (0, 8, 23):
        a, b = (_parts(_case(n), _draw(_case(n))[1])[1] for n in (f"segments_fwd_hw{hw}", f"segments_rev_hw{hw}"))
        assert np.array_equal(a, b)


def test_rasteriser_draws_a_list_and_reports_the_dropped_points():
    from thinktwice_amd import render
    rng = np.random.default_rng(0)
    dl = render.DisplayList(33, 65)
    pts = torch.from_numpy(np.array([[3, 3], [np.nan, 1], [40, 20], [1e30, 0]], np.float32)).cuda()
    bf16 = torch.from_numpy(R.seg_logits(rng)).cuda().bfloat16()                     # a 16-bit storage mode's logits go through .float()
    dl.fill(0, 0, 65, 33, (9, 9, 9)).seg_overlay(bf16, 1, 1, factor=2).polyline(pts, R.IDENT16, (255, 255, 255)).text("OK 1.5", 2, 20)
    ras = render.Rasteriser()
    got = ras.draw(dl)
    want, dropped = render_ref.render(dl)
    assert np.array_equal(got.cpu().numpy(), want) and dropped == 2
    assert ras.status() == [2, 0, 0, 0] and ras.status() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        ras.draw(R.cases("cuda")[-1].dl)                     # one over TT_RENDER_MAX_ITEMS


def test_debug_renderer_frame_equals_the_restatement_of_the_same_tensors():
    from thinktwice_amd import model as tm, params, render, synth
    hw = (128, 256)
    m, cfg = tm.build_thinktwice(dtype="f32x3", final_dim=hw)
    m.load_state_dict(params.init_params(cfg, seed=3))
    batch = synth.make_batch(1, num_points=4096, img_hw=hw, device="cuda")
    with torch.no_grad():
        pred = m.forward_inference(batch)
    dbg = render.DebugRenderer(cfg, device=m.device)
    cloud = batch["points"][0, 0]
    controls = dict(steer=-0.25, throttle=0.5, brake=0.0, speed=3.21, step=17, steer_ctrl=-0.2, steer_traj=-0.3, is_stuck=True)
    gt = pred["pred_wp"][:, -1] * 1.1
    for args in ((batch["img"], pred, cloud, 0, controls, (9.0, -2.5), gt), (batch["img"][0, -1], None, cloud, 0, None, None, None)):
        got = dbg.frame(*args)
        dl = dbg.display_list(*args)
        want, dropped = render_ref.render(dl)
        _, _, W, H = dbg.layout["canvas"]
        assert tuple(got.shape) == (H, W, 3) and got.dtype == torch.uint8
        diff = int((got.cpu().numpy() != want).any(-1).sum())
        print(f"frame {H} x {W}, {len(dl)} items: {diff} pixels differ")
        assert diff == 0 and dbg.status() == [dropped, 0, 0, 0]
    kinds = [it.kind for it in dl.items]
    assert _lib.TT_RENDER_SEG_OVERLAY not in kinds and _lib.TT_RENDER_POLYLINE_DEV not in kinds      # pred None: cameras and cloud only
