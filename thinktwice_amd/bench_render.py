"""Numbers behind profiles/render.txt (one MI355X): render.DebugRenderer's default frame at the full size (four 448 x 896 inputs, seg
and depth heads of a real forward, a 20000-point cloud, six stages of waypoints), the frame through the encoder, and what a
recording AgentTick pays for `render=`.

    python -m thinktwice_amd.bench_render [--repeats 9] [--inner 20] [--ticks 40] [--out profiles/render.txt] [--dump frame.png]

Device times are event pairs around `inner` back-to-back calls, divided by `inner`, the variants interleaved, median of `repeats`;
every figure has its A/A twin (the same call measured again in the same interleaving) next to it.  Nothing here is a pass
criterion."""
import argparse
import statistics
import sys
import tempfile
import time

import numpy as np

from . import _lib, build


def _med(v):
    return statistics.median(v)


def _events(fns, repeats, inner):
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return ms


def compulsory_bytes(dl):
    """What one drawing of `dl` has to move: every source element an item shows, once (the classes / bins of a logit row, x y z of a
    point), and the canvas, written once.  Tables, the list itself and the scratch planes are not counted."""
    read = 0
    for it in dl.items:
        if it.kind == _lib.TT_RENDER_IMAGE_F32:
            read += 12 * -(-it.h // it.scale) * -(-it.w // it.scale)
        elif it.kind == _lib.TT_RENDER_IMAGE_U8:
            read += it.channels * it.h * it.w * it.scale * it.scale
        elif it.kind in (_lib.TT_RENDER_SEG_OVERLAY, _lib.TT_RENDER_DEPTH_MAP):
            read += 4 * it.channels * -(-it.h // it.scale) * -(-it.w // it.scale)
        elif it.kind == _lib.TT_RENDER_POINTS_BEV:
            read += 12 * it.count
        elif it.kind == _lib.TT_RENDER_POLYLINE_DEV:
            read += 8 * it.count
        elif it.kind == _lib.TT_RENDER_TEXT:
            read += it.count
    return read, 3 * dl.height * dl.width


def main(repeats, inner, ticks, dump, emit):
    import torch
    from . import model as tm, params, png_encode, render, synth
    from .agent_tick import AgentTick
    from .ops import check, lib, ptr
    emit(f"build {build.source_fingerprint()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    mdl, cfg = tm.build_thinktwice(dtype="f32x3")
    mdl.load_state_dict(params.init_params(cfg, seed=0))
    batch = synth.make_batch(1, num_points=20000, device="cuda")
    with torch.no_grad():
        pred = mdl.forward_inference(batch)
    dbg = render.DebugRenderer(cfg, device=mdl.device)
    cloud = batch["points"][0, 0]
    controls = dict(steer=-0.25, throttle=0.5, brake=0.0, speed=3.2, step=17, steer_ctrl=-0.2, steer_traj=-0.3, throttle_ctrl=0.5,
                    throttle_traj=0.4, brake_ctrl=0.0, brake_traj=0.0)
    args = (batch["img"], pred, cloud, 0, controls, (9.0, -2.5), None)
    dl = dbg.display_list(*args)
    read, written = compulsory_bytes(dl)
    frame = dbg.frame(*args)
    torch.cuda.synchronize()
    H, W = frame.shape[:2]
    emit(f"\nthe default frame: {H} x {W} x 3 canvas, {len(dl)} items; compulsory bytes {read} read + {written} written")

    table, raw = dl.pack(dbg.raster._table.data_ptr())           # the list as draw() left it on the device
    work, tab = dbg.raster._work, dbg.raster._table

    def call():
        check(lib().tt_render_u8(ptr(frame), H, W, table, ptr(tab), len(dl), ptr(work), work.numel(),
                                 torch.cuda.current_stream().cuda_stream), "tt_render_u8")
    enc = png_encode.PngEncoder()
    enc.encode([frame])
    held = []

    def frame_and_encode():
        held.append(enc.encode_async([dbg.frame(*args)]))
    ms = _events({"call": call, "call_aa": call, "frame": lambda: dbg.frame(*args), "frame_aa": lambda: dbg.frame(*args)}, repeats, inner)
    m = {k: _med(v) for k, v in ms.items()}
    emit(f"  tt_render_u8 alone (the list already uploaded): {1e3 * m['call']:.1f} us (A/A {1e3 * m['call_aa']:.1f}); "
         f"{(read + written) / m['call'] / 1e9 * 1e3:.0f} GB/s of compulsory bytes")
    emit(f"  DebugRenderer.frame (building the list on the host, its upload, the call): {1e3 * m['frame']:.1f} us per frame back to back "
         f"(A/A {1e3 * m['frame_aa']:.1f})")
    ms = _events({"both": frame_and_encode, "both_aa": frame_and_encode, "encode": lambda: held.append(enc.encode_async([frame]))}, repeats, 1)
    for p in held:
        p.result()
    m2 = {k: _med(v) for k, v in ms.items()}
    size = len(enc.encode([frame])[0])
    emit(f"  frame + PngEncoder.encode_async of it (device time up to the copy back): {m2['both']:.2f} ms (A/A {m2['both_aa']:.2f}); the "
         f"encoder alone {m2['encode']:.2f} ms; the file is {size} bytes")
    t = []
    for _ in range(max(repeats, 9)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dbg.frame(*args)
        t.append(1e3 * (time.perf_counter() - t0))
    emit(f"  host time of one DebugRenderer.frame on the caller's thread (idle device): {_med(t):.2f} ms (min {min(t):.2f}, max {max(t):.2f})")
    if dump:
        with open(dump, "wb") as f:
            f.write(enc.encode([frame])[0])

    if ticks > 0:
        with tempfile.TemporaryDirectory() as root:
            rec = png_encode.FrameRecorder(root, max_pending=4)
            mk = lambda **kw: AgentTick(mdl, lag=1, queue_len=2, recorder=rec, **kw)   # noqa: E731
            pair = {"render=None": mk(), "render=None (A/A)": mk(), "render=True": mk(render=dbg), "render=True (A/A)": mk(render=dbg)}
            rng = np.random.default_rng(0)
            raw_frames = torch.from_numpy(synth.raw_camera_frames(seed=17, T=1)[0]).cuda()
            half = np.concatenate([rng.uniform(-8, 30, (10000, 1)), rng.uniform(-19, 19, (10000, 1)), rng.uniform(-4.5, 0.5, (10000, 1)),
                                   rng.uniform(0, 1, (10000, 1))], 1).astype(np.float32)
            targs = (raw_frames, half, np.array([12.0, -3.0]), 0.4, 3.0, np.array([21.0, 11.0]), 2)
            wall = {k: [] for k in pair}
            for i in range(ticks + 4):
                for k, tick in pair.items():                        # alternating, in one process
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    tick.run_step(*targs)
                    host = 1e3 * (time.perf_counter() - t0)
                    torch.cuda.synchronize()
                    if i >= 4:
                        wall[k].append((1e3 * (time.perf_counter() - t0), host, tick.step % 10 == 0))
            rec.close()
            emit(f"\nAgentTick.run_step with a recorder, record_every=10, {ticks} ticks each, alternating (ms: wall synchronised after the "
                 f"tick / host time of run_step alone); {rec.stalls} stalls")
            for k, v in wall.items():
                quiet, loud = [x for x in v if not x[2]], [x for x in v if x[2]]
                emit(f"  {k:<18} not recorded: {_med([x[0] for x in quiet]):.2f} / {_med([x[1] for x in quiet]):.2f}   recorded "
                     f"({len(loud)} ticks): {_med([x[0] for x in loud]):.2f} / {_med([x[1] for x in loud]):.2f}")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--dump", default=None, help="write the frame here as a PNG file")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    rc = main(a.repeats, a.inner, a.ticks, a.dump, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(rc)
