"""The recorder, AgentTick and evaluate with JPEG files and Motion JPEG video, on the GPU, in the manner of test_recorder.py and
test_render_agent.py with their small model and frame sizes.  The codec itself is held to the restatement in
test_jpeg_encode.py; here the files must be the encoder's files of the tensors that were submitted, in the right places and
order, and the defaults must leave a run's files what they were."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_mjpeg_cpu import read_avi  # noqa: E402

pytestmark = pytest.mark.gpu


def _files(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def _pil_psnr(img, quality):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(img).save(out, "JPEG", quality=quality, subsampling=2, optimize=False)
    return _psnr(_decode(out.getvalue()), img)


def test_recorder_writes_png_jpeg_and_video_submissions_of_tiny_frames(tmp_path):
    import jpeg_encode_cases as E
    from thinktwice_amd import jpeg_encode, png_encode
    imgs = [E.camera(24, 40, 3, s) for s in range(4)] + [E.camera(17, 33, 1, 9)]
    dev = [torch.from_numpy(i.copy()).cuda() for i in imgs]
    jenc = jpeg_encode.JpegEncoder(quality=85, subsampling="444")
    rec = png_encode.FrameRecorder(tmp_path, jpeg_encoder=jenc, video_fps=5.0)
    rec.submit({"a/0.png": dev[0], "a/0.jpg": dev[0], "grey/0.JPEG": dev[4]}, {"meta/0.json": b"{}"}, video={"v/drive.avi": dev[1]})
    rec.submit({"a/1.png": dev[1]})
    rec.submit({}, video={"v/drive.avi": dev[2]})
    rec.submit({"a/3.jpg": dev[3]}, video={"v/drive.avi": dev[3]})
    rec.close()
    assert rec.written == rec.submitted == 4
    want_png = png_encode.PngEncoder().encode([dev[0], dev[1]])
    want_jpg = jpeg_encode.JpegEncoder(quality=85, subsampling="444").encode(dev)
    files = _files(tmp_path)
    assert set(files) == {"a/0.png", "a/0.jpg", "grey/0.JPEG", "meta/0.json", "a/1.png", "a/3.jpg", "v/drive.avi"}
    assert [files["a/0.png"], files["a/1.png"]] == want_png
    assert (files["a/0.jpg"], files["grey/0.JPEG"], files["a/3.jpg"]) == (want_jpg[0], want_jpg[4], want_jpg[3])
    avi = read_avi(files["v/drive.avi"])
    assert avi["frames"] == want_jpg[1:4] and avi["avih"][4] == 3 and avi["avih"][8:10] == (40, 24) and avi["avih"][0] == 200000
    assert np.array_equal(_decode(files["a/0.png"]), imgs[0]) and _decode(files["grey/0.JPEG"]).shape == (17, 33)


def test_agent_tick_writes_jpeg_frames_and_a_debug_video_and_the_defaults_write_what_they_wrote(tmp_path):
    from test_agent_tick import _tick_inputs
    from thinktwice_amd import calib, config, dataset, jpeg_encode, model as tm, params, png_encode, render
    from thinktwice_amd.agent_tick import AgentTick
    hw = (128, 256)
    m, cfg = tm.build_thinktwice(dtype="f32x3", final_dim=hw)
    m.load_state_dict(params.init_params(cfg, seed=3))

    class Keeping(render.DebugRenderer):
        """frame() also keeps a copy of the canvas it returns."""

        def frame(self, *a, **k):
            out = super().frame(*a, **k)
            self.__dict__.setdefault("kept", []).append(out.clone())
            return out
    dbg = {k: Keeping(config.model_config(final_dim=hw), device=m.device) for k in ("jpg", "png")}
    recs = {k: png_encode.FrameRecorder(tmp_path / k) for k in ("jpg", "png")}
    common = dict(lag=2, queue_len=4, stuck_threshold=5, final_dim=hw, record_every=2)
    ticks = {"jpg": AgentTick(m, recorder=recs["jpg"], render=dbg["jpg"], image_format="jpg", debug_video=True, **common),
             "png": AgentTick(m, recorder=recs["png"], render=dbg["png"], **common)}
    with pytest.raises(ValueError):
        AgentTick(m, recorder=recs["png"], debug_video=True, **common)           # a video of debug frames needs render
    with pytest.raises(ValueError):
        AgentTick(m, recorder=recs["png"], image_format="bmp", **common)
    inputs = list(_tick_inputs(6))
    runs = {k: [t.run_step(*args) for args in inputs] for k, t in ticks.items()}
    for r in recs.values():
        r.close()
    for (s, th, b, _), (ps, pth, pb, _) in zip(runs["jpg"], runs["png"]):          # the tick itself does not depend on the format
        assert (s, th, b) == (ps, pth, pb)
    files = {k: _files(tmp_path / k) for k in recs}
    names = [dataset.frame_name(n) for n in range(3)]

    # the defaults: the parent's files, byte for byte -- the PNG encoder's output of the same tensors, nothing else
    enc = png_encode.PngEncoder()
    want = {}
    for n, t in zip(names, (0, 2, 4)):
        raw = torch.from_numpy(inputs[t][0]).cuda()
        data = enc.encode([raw[i] for i in range(4)] + [dbg["png"].kept[t // 2]])
        want.update({os.path.join(cam, n + ".png"): d for cam, d in zip(calib.CAMERA_NAMES, data)})
        want[os.path.join("debug", n + ".png")] = data[4]
    assert {k: v for k, v in files["png"].items() if k.endswith(".png")} == want
    assert not [k for k in files["png"] if k.endswith((".jpg", ".avi"))]
    others = {k: v for k, v in files["png"].items() if not k.endswith(".png")}
    assert others == {k: v for k, v in files["jpg"].items() if not k.endswith((".jpg", ".avi"))} and len(others) == 6

    # image_format="jpg": rgb_*/NNNN.jpg of the submitted tensors, no camera or debug PNG; debug.avi: the three frames in order
    assert {k for k in files["jpg"] if k.endswith((".jpg", ".avi", ".png"))} == \
        {os.path.join(cam, n + ".jpg") for cam in calib.CAMERA_NAMES for n in names} | {"debug.avi"}
    jenc = jpeg_encode.JpegEncoder()
    for n, t in zip(names, (0, 2, 4)):
        raw = torch.from_numpy(inputs[t][0]).cuda()
        data = jenc.encode([raw[i] for i in range(4)])
        for i, cam in enumerate(calib.CAMERA_NAMES):
            got = files["jpg"][os.path.join(cam, n + ".jpg")]
            assert got == data[i], (cam, n)
            if i == 0:                                       # within the codec's error: no worse than PIL's own file five steps down
                ours, lower = _psnr(_decode(got), inputs[t][0][i]), _pil_psnr(inputs[t][0][i], 85)
                print(f"{cam}/{n}.jpg: {len(got)} bytes, PSNR {ours:.2f} dB, PIL at quality 85 {lower:.2f} dB")
                assert ours >= lower, (ours, lower)
    avi = read_avi(files["jpg"]["debug.avi"])
    assert avi["frames"] == jenc.encode(dbg["jpg"].kept) and len(avi["frames"]) == 3 and avi["avih"][4] == 3
    assert avi["avih"][0] == 100000                          # 20 Hz / record_every 2 = 10 frames a second
    _, _, W, H = dbg["jpg"].layout["canvas"]
    assert avi["avih"][8:10] == (W, H)
    for f, canvas in zip(avi["frames"], dbg["jpg"].kept):
        assert _psnr(_decode(f), canvas.cpu().numpy()) >= _pil_psnr(canvas.cpu().numpy(), 85)
    assert all(torch.equal(a, b) for a, b in zip(dbg["jpg"].kept, dbg["png"].kept))


def test_frame_dump_writes_one_video_or_jpeg_files_of_two_small_batches(tmp_path):
    from thinktwice_amd import evaluate, jpeg_encode

    class Raster:
        def __init__(self):
            self.drawn = []

        def draw(self, dl):
            self.drawn.append(dl)
            return dl

    class Renderer:
        raster = None

    class Model:
        device = torch.device("cuda", torch.cuda.current_device())

    def canvas(i):
        g = torch.arange(48 * 64 * 3, device="cuda").reshape(48, 64, 3)
        return ((g // 7 + 40 * i) % 256).to(torch.uint8)
    jenc = jpeg_encode.JpegEncoder()
    for fmt in ("avi", "jpg"):
        r = Renderer()
        r.raster = Raster()
        dump = evaluate.FrameDump(Model(), tmp_path / fmt, every=2, renderer=r, render_format=fmt)
        dump.display_list = lambda batch, pred, b, dump=dump: canvas(dump.ordinal)
        for _ in range(2):
            dump.add({}, {"pred_wp": torch.zeros(3, 4, 2)})
        dump.close()
        want = jenc.encode([canvas(i) for i in (0, 2, 4)])
        assert dump.frames == 3 and dump.ordinal == 6
        if fmt == "avi":
            assert os.listdir(tmp_path / fmt) == ["frames.avi"]
            assert read_avi((tmp_path / fmt / "frames.avi").read_bytes())["frames"] == want
        else:
            assert _files(tmp_path / fmt) == {f"{i:06d}.jpg": w for i, w in zip((0, 2, 4), want)}
    with pytest.raises(ValueError):
        evaluate.FrameDump(Model(), tmp_path / "x", every=2, render_format="gif")
