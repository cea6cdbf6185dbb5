"""AgentTick(render=...) and evaluate(render_dir=...) on the GPU: every recorded tick's debug/NNNN.png decodes to the numpy
restatement (tests/render_ref.py) of that tick's display list, the ticks before the queue is full included; without `render` the
recording and the tick are what they were; an evaluation pass writes its frames and its metrics do not move."""
import io
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import render_ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _files(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_agent_tick_records_a_debug_frame_per_tick_and_is_unchanged_without_render(tmp_path):
    from PIL import Image
    from test_agent_tick import _tick_inputs
    from thinktwice_amd import config, dataset, model as tm, params, png, png_encode, render
    from thinktwice_amd.agent_tick import AgentTick
    hw = (128, 256)
    m, cfg = tm.build_thinktwice(dtype="f32x3", final_dim=hw)
    m.load_state_dict(params.init_params(cfg, seed=3))

    class Keeping(render.DebugRenderer):
        """frame() also keeps the display list it drew (its tensors by reference)."""
        lists = []

        def frame(self, *a, **k):
            self.lists.append(self.display_list(*a, **k))
            return super().frame(*a, **k)
    dbg = Keeping(config.model_config(final_dim=hw), device=m.device)
    recs = {k: png_encode.FrameRecorder(tmp_path / k) for k in ("with", "without")}
    ticks = {"with": AgentTick(m, lag=2, queue_len=4, stuck_threshold=5, final_dim=hw, recorder=recs["with"], record_every=1, render=dbg),
             "without": AgentTick(m, lag=2, queue_len=4, stuck_threshold=5, final_dim=hw, recorder=recs["without"], record_every=1,
                                  render=None)}
    assert ticks["without"].renderer is None
    inputs = list(_tick_inputs(6))
    runs = {k: [t.run_step(*args) for args in inputs] for k, t in ticks.items()}
    for r in recs.values():
        r.close()
    for (s, th, b, info), (ps, pth, pb, pinfo) in zip(runs["with"], runs["without"]):       # the same tick, bit for bit
        assert (s, th, b) == (ps, pth, pb) and set(info) == set(pinfo)
        assert torch.equal(info["img"], pinfo["img"]) and torch.equal(info["cloud"], pinfo["cloud"])
        assert (info["pred"] is None) == (pinfo["pred"] is None)
        if info["pred"] is not None:
            for key in ("pred_wp", "mu_branches", "sigma_branches", "_seg_cl", "_depth_cl"):
                assert torch.equal(info["pred"][key], pinfo["pred"][key]), key
    files = {k: _files(tmp_path / k) for k in recs}
    debug = {n for n in files["with"] if n.startswith("debug" + os.sep)}
    assert debug == {os.path.join("debug", dataset.frame_name(t) + ".png") for t in range(6)}
    assert {n: v for n, v in files["with"].items() if n not in debug} == files["without"]     # the same files minus debug/
    assert recs["with"].written == recs["without"].written == 6                                 # one submission per tick

    dec = png.PngDecoder(segments="require", verify=True)
    _, _, W, H = dbg.layout["canvas"]
    assert len(dbg.lists) == 6
    for t, dl in enumerate(dbg.lists):
        data = files["with"][os.path.join("debug", dataset.frame_name(t) + ".png")]
        want, _ = render_ref.render(dl)
        got = dec.decode([data])[0].cpu().numpy().reshape(H, W, 3)
        pil = np.array(Image.open(io.BytesIO(data)))
        print(f"tick {t}: {len(dl)} items, {int((got != want).any(-1).sum())} pixels differ")
        assert np.array_equal(got, want) and np.array_equal(pil, want), t
        kinds = {it.kind for it in dl.items}
        assert (render._lib.TT_RENDER_POLYLINE_DEV in kinds) == (runs["with"][t][3]["pred"] is not None)
    assert runs["with"][0][3]["pred"] is None and runs["with"][5][3]["pred"] is not None     # both kinds of tick were seen
    assert dbg.status() == [0, 0, 0, 0]


def test_evaluate_writes_every_nth_sample_and_its_metrics_do_not_move(tmp_path_factory):
    from PIL import Image
    import dataset_cases as D
    from test_evaluate import HW, VAL_TOWN, _loader, _model
    from thinktwice_amd import evaluate, model as tm, params, render
    tree = D.write_tree(tmp_path_factory.mktemp("tree"))
    _, cfg = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    m3 = _model(params.init_params(cfg, seed=0), "f32x3")
    out = tmp_path_factory.mktemp("frames")
    raws = []
    for kw in ({}, dict(render_dir=out, render_every=2)):
        val = _loader(tree, VAL_TOWN)
        raws.append(evaluate.evaluate(m3, val, raw=True, **kw)[1])
        val.close()
    assert raws[0] == raws[1]                                # integers and f64 sums alike: bit-equal
    samples = raws[0]["num_samples"]
    names = sorted(os.listdir(out))
    assert samples >= 3 and names == [f"{i:06d}.png" for i in range(0, samples, 2)] and len(names) == math.ceil(samples / 2)
    _, _, W, H = render.default_layout(HW)["canvas"]
    for n in names:
        img = np.array(Image.open(out / n))
        assert img.shape == (H, W, 3) and img.any()
