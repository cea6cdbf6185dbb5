"""png_encode.FrameRecorder (the writer thread, back pressure, errors) and AgentTick(recorder=...): what a recorded tick leaves
on disk decodes to what the tick was given, and a tick without a recorder is the tick it was.  The thread and rename logic
also runs on the CPU, with a stub encoder."""
import json
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import png_encode_cases as E  # noqa: E402


class _StubPending:
    def __init__(self, files, gate):
        self._files, self._gate = files, gate

    def result(self):
        self._gate.wait(10)
        return self._files


class _StubEncoder:
    """encode_async -> one b"png:<tag>" per image, ready once `gate` is set."""

    def __init__(self):
        self.gate = threading.Event()

    def encode_async(self, images):
        return _StubPending([b"png:" + str(i).encode() for i in images], self.gate)


def test_recorder_thread_renames_blocks_and_surfaces_errors_cpu(tmp_path):
    from thinktwice_amd import png_encode
    enc = _StubEncoder()
    rec = png_encode.FrameRecorder(tmp_path / "run", encoder=enc, max_pending=1)
    rec.submit({"a/0000.png": 1, "b/0000.png": 2}, {"meta/0000.json": b"{}"})
    assert rec.stalls == 0 and not (tmp_path / "run" / "a" / "0000.png").exists()      # the writer waits for the encoder
    threading.Timer(0.05, enc.gate.set).start()
    rec.submit({"a/0001.png": 3})                                                      # blocks until the first one is written
    assert rec.stalls == 1 and (tmp_path / "run" / "a" / "0000.png").read_bytes() == b"png:1"
    rec.submit({}, {"only/file.bin": b"xyz"})
    rec.close()
    rec.close()                                                                         # idempotent
    root = tmp_path / "run"
    assert (root / "b" / "0000.png").read_bytes() == b"png:2" and (root / "a" / "0001.png").read_bytes() == b"png:3"
    assert (root / "meta" / "0000.json").read_bytes() == b"{}" and (root / "only" / "file.bin").read_bytes() == b"xyz"
    assert rec.submitted == rec.written == 3
    assert not [f for _, _, fs in os.walk(root) for f in fs if ".tmp" in f]             # every temporary name was renamed
    with pytest.raises(RuntimeError):
        rec.submit({"a/0002.png": 4})
    outside = png_encode.FrameRecorder(tmp_path / "x", encoder=enc)
    with pytest.raises(ValueError):
        outside.submit({"../escape.png": 1})
    outside.close()

    blocked = tmp_path / "file"
    blocked.write_bytes(b"")                                                            # a root that cannot hold directories
    bad = png_encode.FrameRecorder(blocked, encoder=enc, max_pending=2)
    bad.submit({"a/0000.png": 1})
    with pytest.raises(OSError):
        bad.close()


@pytest.mark.gpu
def test_recorder_writes_mixed_shapes_and_counts_stalls(tmp_path):
    from thinktwice_amd import png, png_encode
    rec = png_encode.FrameRecorder(tmp_path, max_pending=1)
    picks = [c for c in E.cases() if c[0].startswith(("camera", "tags", "image_17"))][:6]
    tensors = {f"s{k}/{i:04d}.png": torch.from_numpy(picks[2 * k + i][1].copy()).cuda() for k in range(3) for i in range(2)}
    for k in range(3):
        rec.submit({n: t for n, t in tensors.items() if n.startswith(f"s{k}/")}, {f"s{k}/note.txt": b"%d" % k})
    rec.close()
    assert rec.written == 3 and rec.stalls >= 1              # three submissions through one slot: the later ones had to wait
    dec = png.PngDecoder(segments="require", verify=True)
    for name, t in tensors.items():
        got = dec.decode([(tmp_path / name).read_bytes()])[0]
        assert torch.equal(got.reshape(t.shape), t), name
    assert (tmp_path / "s2" / "note.txt").read_bytes() == b"2"

    blocked = tmp_path / "blocked"
    blocked.write_bytes(b"")
    bad = png_encode.FrameRecorder(blocked, encoder=rec.encoder)
    bad.submit({"a/0000.png": next(iter(tensors.values()))})
    with pytest.raises(OSError):
        bad.close()


@pytest.mark.gpu
def test_agent_tick_records_every_second_tick_and_is_unchanged_without_a_recorder(tmp_path):
    from test_agent_tick import _tick_inputs
    from thinktwice_amd import calib, dataset, model as tm, params, png, png_encode
    from thinktwice_amd.agent_tick import AgentTick
    hw = (128, 256)
    m, cfg = tm.build_thinktwice(dtype="f32x3", final_dim=hw)
    m.load_state_dict(params.init_params(cfg, seed=3))
    rec = png_encode.FrameRecorder(tmp_path)
    ticks = {"plain": AgentTick(m, lag=2, queue_len=4, stuck_threshold=5, final_dim=hw),
             "none": AgentTick(m, lag=2, queue_len=4, stuck_threshold=5, final_dim=hw, recorder=None, record_every=2),
             "rec": AgentTick(m, lag=2, queue_len=4, stuck_threshold=5, final_dim=hw, recorder=rec, record_every=2)}
    inputs = list(_tick_inputs(6))
    runs = {k: [t.run_step(*args) for args in inputs] for k, t in ticks.items()}
    rec.close()
    for k in ("none", "rec"):                                # the controls and the info of the same ticks, bit for bit
        for (s, th, b, info), (ps, pth, pb, pinfo) in zip(runs[k], runs["plain"]):
            assert (s, th, b) == (ps, pth, pb) and set(info) == set(pinfo)
            assert torch.equal(info["img"], pinfo["img"]) and torch.equal(info["cloud"], pinfo["cloud"])
            for key in set(info) - {"img", "cloud", "pred", "target_point"}:
                assert info[key] == pinfo[key], key
            if info["pred"] is not None:
                for key in ("pred_wp", "mu_branches", "sigma_branches"):
                    assert torch.equal(info["pred"][key], pinfo["pred"][key]), key
    dec = png.PngDecoder(segments="require", verify=True)
    assert rec.written == 3
    for t in (0, 2, 4):
        name = dataset.frame_name(t // 2)
        frames, (s, th, b, info) = inputs[t][0], runs["rec"][t]
        files = [(tmp_path / cam / f"{name}.png").read_bytes() for cam in calib.CAMERA_NAMES]
        assert torch.equal(dec.decode(files).cpu(), torch.from_numpy(frames))
        cloud = dataset.load_cloud((tmp_path / "lidar" / f"{name}.npy").read_bytes())
        assert np.array_equal(cloud, info["cloud"].cpu().numpy())
        meta = json.loads((tmp_path / "meta" / f"{name}.json").read_text())
        assert (meta["steer"], meta["throttle"], meta["brake"]) == (s, th, b) and meta["speed"] == inputs[t][4]
        if t >= 4:                                           # a live tick: the two heads, the stuck counter, the target point
            for key in ("steer_ctrl", "steer_traj", "throttle_ctrl", "throttle_traj", "brake_ctrl", "brake_traj", "stuck_detector"):
                assert meta[key] == info[key], key
            assert meta["target_point"] == [float(v) for v in info["target_point"]]
    assert not (tmp_path / "rgb_front" / f"{dataset.frame_name(3)}.png").exists()
