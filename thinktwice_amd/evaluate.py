"""Open-loop evaluation of a checkpoint on recorded frames: task metrics accumulated on the device (csrc/eval_metrics.hip; the
contract of the entries is in include/thinktwice_hip.h) and, for two precision modes of one state_dict, how far their outputs
and their metrics differ.

    python -m thinktwice_amd.evaluate --data-root <dir> --metadata <dataset_metadata.pkl> --load-from ckpt.pth \\
        [--dtype f32x3h] [--against f32] [--towns town02_val ...] [--batch-size 8] [--out metrics.json]
    python -m torch.distributed.run --nproc_per_node 8 -m thinktwice_amd.evaluate ...     # the loader shards, the result is merged

    window = MetricWindow(model.device, num_classes=12, depth_bins=80, stages=6)
    window.add(batch, pred)             # three launches, nothing waits for the device
    summary = summarize(window.close().result())

The metric definitions are this project's own (the reference reports the 23 loss means of custom_multi_gpu_test and the
closed-loop Driving Score, which needs a simulator).  One convention is the reference's: which label a seg / depth cell is
compared with -- get_downsampled_gt_seg / get_downsampled_gt_depth (encoder_decoder_framework.py:443-491), the cells the two
losses supervise.  The closed-loop control action is out of scope: tt_action_post needs the PID state of a driven route.
"""
import argparse
import json
import math
import os
from collections import OrderedDict

# the A22 output keys compare_modes reports (tests/test_forward.py's)
OUTPUT_KEYS = ("pred_wp", "mu_branches", "sigma_branches", "future_mu", "future_sigma", "pred_speed", "pred_value_traj",
               "pred_value_ctrl", "pred_features_traj", "pred_features_ctrl", "bev_feature", "refine_BEV_feature",
               "refine_flattned_BEV_feature", "refine_future_BEV_feature")
STAGE_TERMS = ("wp_ade", "wp_fde", "wp_long", "wp_lat", "mu_l1_0", "mu_l1_1", "sigma_l1_0", "sigma_l1_1")     # sums[8 s + j]
DEPTH_COUNTS = ("n_fg", "n_top1", "n_within1", "sum_abs_bins", "nonfinite")
DTYPES = ("f32", "f32x3", "f32x3h", "bf16", "f16")
# CARLA's semantic tags of configs/thinktwice.py:108 (public: the simulator's documentation)
_TAG_NAMES = {1: "building", 4: "pedestrian", 5: "pole", 6: "road_line", 7: "road", 8: "sidewalk", 10: "vehicle", 12: "traffic_sign",
              18: "traffic_light"}


def seg_class_names(seg_label_idxs=None, num_classes=12, traffic_light_tag=18):
    """The name of every seg class as labels.seg_decode_conf numbers them: a tag's class is its position in `seg_label_idxs`
    (the first shares class 0 with the background), the traffic-light tag's position is followed by its red and green class."""
    if seg_label_idxs is None:
        from .data_config import DATA
        seg_label_idxs = DATA["seg_label_idxs"]
    names = []
    for i, tag in enumerate(seg_label_idxs):
        name = _TAG_NAMES.get(tag, f"tag{tag}")
        names.append(f"background_{name}" if i == 0 else name)
        if tag == traffic_light_tag:
            names += [name + "_red", name + "_green"]
    names = names[:num_classes]
    return names + [f"class{i}" for i in range(len(names), num_classes)]


def _div(a, b):
    return a / b if b else float("nan")


def summarize(raw, class_names=None, d_step=None):
    """Pure host arithmetic: the raw accumulators (`PendingMetrics.result()` / `MetricWindow.merge_ranks`) -> an OrderedDict of
    metrics.  Per stage s: wp_ade_s, wp_fde_s, wp_long_s, wp_lat_s, mu_l1_0_s, mu_l1_1_s, sigma_l1_0_s, sigma_l1_1_s (means over the
    finite samples), speed_mae; seg_iou (per class name; None where the union is empty), seg_miou over the others, seg_pixel_acc;
    depth_top1, depth_within1, depth_mae_m (= sum_abs_bins * d_step / n_fg); the counters.  A mean over nothing is NaN."""
    out = OrderedDict()
    n = int(raw["num_samples"])
    sums = [float(v) for v in raw["dec_sums"]]
    stages = (len(sums) - 1) // 8
    for s in range(stages):
        for j, name in enumerate(STAGE_TERMS):
            out[f"{name}_{s}"] = _div(sums[8 * s + j], n)
    out["speed_mae"] = _div(sums[8 * stages], n)
    conf = raw.get("seg_conf")
    if conf is not None:
        C = len(conf)
        names = list(class_names) if class_names is not None else seg_class_names(num_classes=C)
        iou, total, diag = OrderedDict(), 0, 0
        for c in range(C):
            tp = int(conf[c][c])
            union = sum(int(conf[c][k]) for k in range(C)) + sum(int(conf[k][c]) for k in range(C)) - tp
            iou[names[c]] = tp / union if union else None
            diag += tp
            total += sum(int(conf[c][k]) for k in range(C))
        have = [v for v in iou.values() if v is not None]
        out["seg_iou"] = iou
        out["seg_miou"] = sum(have) / len(have) if have else float("nan")
        out["seg_pixel_acc"] = _div(diag, total)
        out["seg_bad_label"], out["seg_nonfinite"] = int(raw["seg_bad_label"]), int(raw["seg_nonfinite"])
    dep = raw.get("depth")
    if dep is not None:
        d = dict(zip(DEPTH_COUNTS, (int(v) for v in dep)))
        step = float(raw.get("d_step", d_step if d_step is not None else float("nan")))
        out["depth_top1"], out["depth_within1"] = _div(d["n_top1"], d["n_fg"]), _div(d["n_within1"], d["n_fg"])
        out["depth_mae_m"] = _div(d["sum_abs_bins"] * step, d["n_fg"])
        out["depth_n_fg"], out["depth_nonfinite"] = d["n_fg"], d["nonfinite"]
    out["nonfinite"] = int(raw["dec_nonfinite"])
    out["num_samples"] = n
    return out


def scalar_metrics(summary):
    """The flat float-valued part of a summary (what joins a log line and what `save_best` may name): every number, the
    per-class IoUs as seg_iou_<name> (absent where None)."""
    flat = OrderedDict()
    for k, v in summary.items():
        if k == "seg_iou":
            for name, x in v.items():
                if x is not None:
                    flat[f"seg_iou_{name}"] = x
        elif isinstance(v, (int, float)) and k != "num_samples":
            flat[k] = v
    return flat


class PendingMetrics:
    """A closed MetricWindow on its way to the host: `ready()` never blocks, `result()` waits for the copy if it has to and
    returns the raw accumulators as a dict (integers as Python ints, the f64 sums as floats)."""

    def __init__(self, window, host, event, keep):
        self._layout, self._host, self._event, self._keep = window._layout(), host, event, keep
        self._result = None

    def ready(self):
        return self._result is not None or self._event.query()

    def result(self):
        if self._result is None:
            self._event.synchronize()
            self._result = self._layout.unpack(self._host)
            self._keep = None
        return self._result


class _Layout:
    """Where everything lives in a MetricWindow's buffer of 8-byte slots: [seg: C*C + 2][depth: 5][counts: 2][sums: 8 S + 1]."""

    def __init__(self, num_classes, depth_bins, stages, d_step):
        self.C, self.D, self.S, self.d_step = int(num_classes), int(depth_bins), int(stages), d_step
        self.seg = 0
        self.depth = self.seg + self.C * self.C + 2
        self.counts = self.depth + 5
        self.sums = self.counts + 2
        self.size = self.sums + 8 * self.S + 1

    def unpack(self, vec):
        """int64 host tensor (the buffer's bits) -> the raw dict."""
        import torch
        ints = vec.tolist()
        C = self.C
        raw = OrderedDict()
        raw["seg_conf"] = [ints[r * C:(r + 1) * C] for r in range(C)]
        raw["seg_bad_label"], raw["seg_nonfinite"] = ints[C * C], ints[C * C + 1]
        raw["depth"] = ints[self.depth:self.depth + 5]
        raw["num_samples"], raw["dec_nonfinite"] = ints[self.counts], ints[self.counts + 1]
        raw["dec_sums"] = vec[self.sums:self.size].contiguous().view(torch.float64).tolist()
        if self.d_step is not None:
            raw["d_step"] = float(self.d_step)
        return raw


class MetricWindow:
    """Device accumulators of the task metrics of one evaluation: int64 counts and f64 sums in ONE buffer this object owns.
    `add(batch, pred)` queues tt_eval_decoder and, when the model has the heads and the batch the labels, tt_eval_seg_confusion and
    tt_eval_depth_bins; `close()` hands the buffer over (`PendingMetrics`) and starts the next window.  Nothing here waits for the
    device.  `seg_factor`, `depth_factor`, `d_bound`: the model's seg_downsample_factor, downsample_factor and d_bound (taken
    from `model=` when given)."""

    def __init__(self, device, num_classes=12, depth_bins=None, stages=6, class_names=None, model=None, seg_factor=2,
                 depth_factor=16, d_bound=None):
        import torch
        self.device = torch.device(device)
        self.use_seg = self.use_depth = True
        if model is not None:
            seg_factor, depth_factor = model.seg_downsample_factor, model.downsample_factor
            d_bound = model.d_bound if d_bound is None else d_bound
            self.use_seg, self.use_depth = bool(model.use_seg), bool(model.use_depth)
        self.seg_factor, self.depth_factor = int(seg_factor), int(depth_factor)
        self.d_bound = None if d_bound is None else tuple(float(v) for v in d_bound)
        if depth_bins is None:
            if self.d_bound is None:
                raise ValueError("MetricWindow: depth_bins or d_bound (or model=)")
            depth_bins = int((self.d_bound[1] - self.d_bound[0]) / self.d_bound[2])
        self.num_classes, self.depth_bins, self.stages = int(num_classes), int(depth_bins), int(stages)
        self.class_names = list(class_names) if class_names is not None else seg_class_names(num_classes=self.num_classes)
        if len(self.class_names) != self.num_classes:
            raise ValueError(f"MetricWindow: {len(self.class_names)} class names for {self.num_classes} classes")
        lay = self._layout()
        self.buf = torch.zeros(lay.size, dtype=torch.int64, device=self.device)
        self._sums = self.buf[lay.sums:].view(torch.float64)
        self.adds = 0

    def _layout(self):
        return _Layout(self.num_classes, self.depth_bins, self.stages, None if self.d_bound is None else self.d_bound[2])

    def _f32(self, t):
        import torch
        t = t.to(self.device, torch.float32)
        return t if t.is_contiguous() else t.contiguous()

    def add(self, batch, pred):
        """One batch: `batch` a loader batch (waypoints, action_mu, action_sigma, speed; seg / depth labels where it has them),
        `pred` the dict of `forward_inference` for it."""
        from ._lib import check, cur_stream, lib, ptr
        L, st, lay = lib(), cur_stream(self.device), self._layout()
        wp, mu, sg, sp = (self._f32(pred[k]) for k in ("pred_wp", "mu_branches", "sigma_branches", "pred_speed"))
        B, S = wp.shape[0], wp.shape[1]
        if S != self.stages or tuple(wp.shape[2:]) != (4, 2) or tuple(mu.shape) != (B, S, 2) or tuple(sg.shape) != (B, S, 2) \
                or sp.numel() != B:
            raise ValueError(f"MetricWindow.add: pred_wp {tuple(wp.shape)}, mu_branches {tuple(mu.shape)}, pred_speed "
                             f"{tuple(sp.shape)} for {self.stages} stages")
        gwp, gmu, gsg, gsp = (self._f32(batch[k]) for k in ("waypoints", "action_mu", "action_sigma", "speed"))
        if tuple(gwp.shape) != (B, 4, 2) or tuple(gmu.shape) != (B, 2) or tuple(gsg.shape) != (B, 2) or gsp.numel() != B:
            raise ValueError(f"MetricWindow.add: waypoints {tuple(gwp.shape)}, action_mu {tuple(gmu.shape)}, speed "
                             f"{tuple(gsp.shape)} for a batch of {B}")
        check(L.tt_eval_decoder(ptr(wp), ptr(mu), ptr(sg), ptr(sp), ptr(gwp), ptr(gmu), ptr(gsg), ptr(gsp), B, S,
                                ptr(self._sums), ptr(self.buf[lay.counts:]), st), "tt_eval_decoder")
        if self.use_seg and pred.get("_seg_cl") is not None and batch.get("seg") is not None:
            seg, lab = self._f32(pred["_seg_cl"]), self._f32(batch["seg"])
            b, n, H, W = lab.shape
            f = self.seg_factor
            if tuple(seg.shape[:3]) != (b * n, H // f, W // f):
                raise ValueError(f"MetricWindow.add: seg logits {tuple(seg.shape)} for labels {tuple(lab.shape)} at factor {f}")
            check(L.tt_eval_seg_confusion(ptr(seg), seg.shape[-1], self.num_classes, ptr(lab), b * n, H, W, f,
                                          ptr(self.buf[lay.seg:]), st), "tt_eval_seg_confusion")
        if self.use_depth and pred.get("_depth_cl") is not None and batch.get("depth") is not None:
            if self.d_bound is None:
                raise ValueError("MetricWindow.add: depth logits and labels but no d_bound")
            dep, gt = self._f32(pred["_depth_cl"]), self._f32(batch["depth"])
            b, n, H, W = gt.shape
            f = self.depth_factor
            if tuple(dep.shape[:3]) != (b * n, H // f, W // f):
                raise ValueError(f"MetricWindow.add: depth logits {tuple(dep.shape)} for maps {tuple(gt.shape)} at factor {f}")
            check(L.tt_eval_depth_bins(ptr(dep), dep.shape[-1], self.depth_bins, ptr(gt), b * n, H, W, f, self.d_bound[0],
                                       self.d_bound[2], ptr(self.buf[lay.depth:]), st), "tt_eval_depth_bins")
        self.adds += 1

    def close(self):
        """Queue the hand-over of what was gathered and start the next window: a device copy, zeroing, one device-to-pinned copy,
        an event.  Never waits."""
        import torch
        out = self.buf.clone()
        self.buf.zero_()
        host = torch.empty(out.numel(), dtype=torch.int64, pin_memory=True)
        host.copy_(out, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(self.device))
        self.adds = 0
        return PendingMetrics(self, host, event, out)

    def merge_ranks(self, raw, dist=None):
        """One all_gather (of the raw accumulators, as an object: a few hundred numbers); integers add exactly, the f64 sums add in rank order, so every rank holds the same
        result.  `raw`: this rank's `close().result()`.  No process group (or a world of 1): `raw` itself."""
        from .runner import _dist
        dist = _dist(dist)
        if dist is None or dist.get_world_size() == 1:
            return raw
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, raw)
        return merge_raw(parts)

    def summarize(self, raw):
        return summarize(raw, self.class_names)


def merge_raw(parts):
    """The raw accumulators of several ranks (or windows), in rank order, as one: integer counts add exactly; each f64 sum is
    part 0's plus part 1's plus ..., in that order."""
    out = OrderedDict()
    first = parts[0]
    C = len(first["seg_conf"])
    out["seg_conf"] = [[sum(int(p["seg_conf"][r][c]) for p in parts) for c in range(C)] for r in range(C)]
    for k in ("seg_bad_label", "seg_nonfinite"):
        out[k] = sum(int(p[k]) for p in parts)
    out["depth"] = [sum(int(p["depth"][i]) for p in parts) for i in range(5)]
    for k in ("num_samples", "dec_nonfinite"):
        out[k] = sum(int(p[k]) for p in parts)
    sums = list(first["dec_sums"])
    for p in parts[1:]:
        sums = [a + float(b) for a, b in zip(sums, p["dec_sums"])]
    out["dec_sums"] = sums
    if "d_step" in first:
        out["d_step"] = first["d_step"]
    return out


def window_for(model, class_names=None):
    """The MetricWindow of a model: its device, heads and label geometry; the stages are the decoder's (coarse + refinements)."""
    stages = int(getattr(model.decoder, "refine_num", 5)) + 1 if hasattr(model, "decoder") else 6
    return MetricWindow(model.device, num_classes=12, stages=stages, class_names=class_names, model=model)


class FrameDump:
    """Every `every`-th sample of a pass as a debug frame `root/NNNNNN.png`, numbered by the sample's ordinal in this process's
    pass: drawn by render.DebugRenderer from the forward the metrics read, with the batch's expert waypoints in white and its target
    point as a red disc (both read on the device), written through a png_encode.FrameRecorder.  Nothing here waits for the device
    but the recorder's own writer thread.  render_format: "png"; "jpg": `root/NNNNNN.jpg`, baseline JPEG written on the device
    (jpeg_encode.JpegEncoder); "avi": ONE Motion JPEG file `root/frames.avi` of all the frames in the pass's order
    (jpeg_encode.MjpegWriter; with several ranks every rank's directory holds its own)."""

    FORMATS = ("png", "jpg", "avi")

    def __init__(self, model, root, every, renderer=None, recorder=None, render_format="png"):
        from . import png_encode
        if int(every) < 1:
            raise ValueError(f"render_every {every} must be at least 1")
        if render_format not in self.FORMATS:
            raise ValueError(f"render_format: {render_format!r} not in {self.FORMATS}")
        self.render_format = render_format
        self.every, self.ordinal, self.frames = int(every), 0, 0
        self.device, self.renderer = model.device, renderer            # (made at the first batch, for the size of its images)
        self.recorder = recorder or png_encode.FrameRecorder(root, png_encode.PngEncoder(device=model.device))

    def add(self, batch, pred):
        if self.renderer is None:
            from . import config, render
            self.renderer = render.DebugRenderer(config.model_config(final_dim=tuple(batch["img"].shape[-2:])), device=self.device)
        B = pred["pred_wp"].shape[0]
        for b in range(B):
            if self.ordinal % self.every == 0:
                dl = self.display_list(batch, pred, b)
                frame = self.renderer.raster.draw(dl)
                if self.render_format == "avi":
                    self.recorder.submit({}, video={"frames.avi": frame})
                else:
                    self.recorder.submit({f"{self.ordinal:06d}.{self.render_format}": frame})
                self.frames += 1
            self.ordinal += 1

    def display_list(self, batch, pred, b):
        r = self.renderer
        points = batch.get("points")
        dl = r.display_list(batch["img"], pred, None if points is None else points[b, 0], b=b, gt_wp=batch.get("waypoints"),
                            controls={"step": self.ordinal})
        if batch.get("target_point") is not None:
            dl.polyline(batch["target_point"][b:b + 1], r.matrices["target"], (255, 64, 64), half_width=0, radius=72, clip=r.layout["bev"])
        return dl

    def close(self):
        self.recorder.close()


def evaluate(model, loader, dist=None, window=None, raw=False, render_dir=None, render_every=0, render_format="png"):
    """`model.forward_inference(batch)` under no_grad on every batch of `loader` (a DeviceBatchLoader(train=False)): the inference
    path, no teacher pass, in whatever `dtype` mode the model was built.  -> the summary (merged over the ranks of `dist`);
    `raw=True`: (summary, raw accumulators).  render_dir with render_every = N > 0: every N-th sample also becomes a debug frame
    (`FrameDump`; render_format "png", "jpg" or "avi"), from the same forward; the metrics are the bits they are without it."""
    import torch
    window = window or window_for(model)
    dump = (FrameDump(model, render_dir, render_every, render_format=render_format)
            if render_dir is not None and int(render_every) > 0 else None)
    iters = 0
    try:
        with torch.no_grad():
            for batch in loader:
                pred = model.forward_inference(batch)
                window.add(batch, pred)
                if dump is not None:
                    dump.add(batch, pred)
                iters += 1
    finally:
        if dump is not None:
            dump.close()
    if iters == 0:
        raise ValueError("evaluate: the loader gave no batch")
    acc = window.merge_ranks(window.close().result(), dist)
    summary = window.summarize(acc)
    return (summary, acc) if raw else summary


class PairWindow:
    """Device accumulators of compare_modes: per output key [bits of max |a - b|, bits of max |a|, non-finite elements], the
    waypoint distance [max, sum | points, non-finite points] and the seg cells [differing, compared, non-finite]."""

    def __init__(self, device, keys=OUTPUT_KEYS, num_classes=12):
        import torch
        self.device, self.keys, self.num_classes = torch.device(device), tuple(keys), int(num_classes)
        n = 3 * len(self.keys)
        self.buf = torch.zeros(n + 2 + 2 + 3, dtype=torch.int64, device=self.device)
        self._wp, self._wp_counts, self._seg = n, n + 2, n + 4

    def add(self, pred_a, pred_b):
        import torch
        from ._lib import check, cur_stream, lib, ptr
        L, st = lib(), cur_stream(self.device)

        def f32(t):
            t = t.to(self.device, torch.float32)
            return t if t.is_contiguous() else t.contiguous()
        for i, k in enumerate(self.keys):
            a, b = f32(pred_a[k]), f32(pred_b[k])
            if a.shape != b.shape:
                raise ValueError(f"PairWindow.add: {k}: {tuple(a.shape)} against {tuple(b.shape)}")
            check(L.tt_eval_pair_deviation(ptr(a), ptr(b), a.numel(), ptr(self.buf[3 * i:]), st), "tt_eval_pair_deviation")
        a, b = f32(pred_a["pred_wp"]), f32(pred_b["pred_wp"])
        check(L.tt_eval_pair_wp(ptr(a), ptr(b), a.numel() // 2, ptr(self.buf[self._wp:].view(torch.float64)),
                                ptr(self.buf[self._wp_counts:]), st), "tt_eval_pair_wp")
        if pred_a.get("_seg_cl") is not None and pred_b.get("_seg_cl") is not None:
            a, b = f32(pred_a["_seg_cl"]), f32(pred_b["_seg_cl"])
            if a.shape != b.shape:
                raise ValueError(f"PairWindow.add: seg maps {tuple(a.shape)} against {tuple(b.shape)}")
            check(L.tt_eval_pair_seg(ptr(a), ptr(b), a.shape[-1], self.num_classes, a.numel() // a.shape[-1],
                                     ptr(self.buf[self._seg:]), st), "tt_eval_pair_seg")

    def result(self):
        """Blocking: the report of what was added."""
        import struct
        import torch
        host = self.buf.cpu()
        ints = host.tolist()

        def f32(bits):
            return struct.unpack("<f", struct.pack("<I", bits & 0xFFFFFFFF))[0]
        out = OrderedDict()
        rel = OrderedDict()
        for i, k in enumerate(self.keys):
            d, m, nf = f32(ints[3 * i]), f32(ints[3 * i + 1]), ints[3 * i + 2]
            rel[k] = OrderedDict(max_abs_diff=d, max_abs=m, rel=_div(d, m), nonfinite=nf)
        out["outputs"] = rel
        mx, sm = host[self._wp:self._wp + 2].contiguous().view(torch.float64).tolist()
        pts, bad = ints[self._wp_counts], ints[self._wp_counts + 1]
        out["wp_l2_max_mm"], out["wp_l2_mean_mm"] = mx * 1e3, _div(sm, pts) * 1e3
        out["wp_points"], out["wp_nonfinite"] = pts, bad
        differ, seen, nf = ints[self._seg:self._seg + 3]
        out["seg_cells_differ"], out["seg_cells"], out["seg_cells_nonfinite"] = differ, seen, nf
        out["seg_differ_share"] = _div(differ, seen)
        return out


def compare_modes(model_a, model_b, loader):
    """Two models built from one state_dict with different `dtype` run on every batch of `loader`.  -> per A22 output key
    max |a - b| / max |a| (with both maxima), the waypoint L2 distance's max and mean in millimetres, the share of seg cells whose
    class differs, both models' metric summaries (`a`, `b`) and their differences (`delta`: b - a for every number)."""
    import torch
    wa, wb = window_for(model_a), window_for(model_b)
    pair = PairWindow(model_a.device)
    iters = 0
    with torch.no_grad():
        for batch in loader:
            pa = model_a.forward_inference(batch)
            pb = model_b.forward_inference(batch)
            pair.add(pa, pb)
            wa.add(batch, pa)
            wb.add(batch, pb)
            iters += 1
    if iters == 0:
        raise ValueError("compare_modes: the loader gave no batch")
    out = pair.result()
    out["a"], out["b"] = wa.summarize(wa.close().result()), wb.summarize(wb.close().result())
    fa, fb = scalar_metrics(out["a"]), scalar_metrics(out["b"])
    out["delta"] = OrderedDict((k, fb[k] - fa[k]) for k in fa if k in fb)
    return out


# ------------------------------------------------------------------------------------------------------------------- CLI
def parse_args(argv=None):
    from . import data_config as dc
    ap = argparse.ArgumentParser(prog="python -m thinktwice_amd.evaluate", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data-root", required=True, help="the directory the dataset's route paths are relative to")
    ap.add_argument("--metadata", default=None, help="dataset_metadata.pkl (default: <data-root>/../dataset/dataset_metadata.pkl)")
    ap.add_argument("--load-from", default=None, help="a checkpoint or a bare state_dict (default: init_params, for dry runs)")
    ap.add_argument("--dtype", choices=DTYPES, default="f32x3h", help="the model's precision mode")
    ap.add_argument("--against", choices=DTYPES, default=None, help="also run this mode on the same frames and report the deltas")
    ap.add_argument("--towns", nargs="+", default=None, help="the towns to evaluate (default: the split's validation towns)")
    ap.add_argument("--batch-size", type=int, default=dc.BATCH_SIZE_PER_GPU)
    ap.add_argument("--final-dim", type=int, nargs=2, default=None, metavar=("H", "W"), help="reduced image size (default 448 896)")
    ap.add_argument("--dev", action="store_true", help="the reference's is_dev split")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="write the result here as JSON (rank 0)")
    ap.add_argument("--render", default=None, metavar="DIR", help="write debug frames DIR/NNNNNN.png (DIR/rankK with several ranks)")
    ap.add_argument("--render-every", type=int, default=0, metavar="N", help="every N-th sample of the pass gets a frame")
    ap.add_argument("--render-format", default="png", choices=FrameDump.FORMATS,
                    help="png or jpg: one file a frame; avi: one Motion JPEG video DIR/frames.avi")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        ap.error("--batch-size must be >= 1")
    if (args.render is None) != (args.render_every <= 0):
        ap.error("--render DIR and --render-every N (>= 1) go together")
    if args.render is not None and args.against is not None:
        ap.error("--render draws the frames of one mode: not with --against")
    if args.against is not None and args.against == args.dtype:
        ap.error("--against names the mode of --dtype")
    return args


def _torch_dtype(name):
    import torch
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}.get(name, name)


def _jsonable(x):
    if isinstance(x, dict):
        return OrderedDict((k, _jsonable(v)) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, float) and not math.isfinite(x):
        return None
    return x


def main(argv=None):
    args = parse_args(argv)
    import datetime
    import torch
    import torch.distributed as dist
    from . import data_config as dc, dataset, model as tm, params
    from .loader import DeviceBatchLoader
    if not torch.cuda.is_available():
        raise SystemExit("thinktwice_amd.evaluate needs a GPU: there is no CPU path")
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    started = False
    if world > 1 and not dist.is_initialized():
        dist.init_process_group(backend="nccl", device_id=device, timeout=datetime.timedelta(minutes=4))
        started = True
    try:
        cfg = dc.data_config(dev=args.dev)
        towns = list(args.towns) if args.towns else cfg["val_town"]
        final_dim = tuple(args.final_dim) if args.final_dim else None
        overrides = {} if final_dim is None else {"final_dim": final_dim}
        metadata = args.metadata or os.path.join(args.data_root, "..", "dataset", "dataset_metadata.pkl")

        def build(dtype):
            m, mcfg = tm.build_thinktwice(dtype=_torch_dtype(dtype), device=device, **overrides)
            if args.load_from:
                sd = torch.load(args.load_from, map_location="cpu", weights_only=False)
                sd = sd.get("state_dict", sd)
            else:
                sd = params.init_params(mcfg, seed=args.seed)
            m.load_state_dict({k: (v.to(device) if torch.is_tensor(v) else v) for k, v in sd.items()})
            m.eval()
            return m
        index = dataset.DatasetIndex(metadata, towns, cfg, root=args.data_root)
        loader = DeviceBatchLoader(index, cfg, dc.ida_aug_conf(final_dim), device=device, train=False, rank=rank, world=world,
                                   batch_size=args.batch_size, seed=args.seed)
        try:
            model = build(args.dtype)
            result = OrderedDict(dtype=args.dtype, towns=towns, world=world)
            if args.against is None:
                render_dir = args.render if args.render is None or world == 1 else os.path.join(args.render, f"rank{rank}")
                result["metrics"] = evaluate(model, loader, render_dir=render_dir, render_every=args.render_every,
                                             render_format=args.render_format)
            else:
                if world > 1:
                    raise SystemExit("--against compares two modes on one rank's frames: run it without torch.distributed.run")
                result["against"] = args.against
                result["compare"] = compare_modes(model, build(args.against), loader)
                result["metrics"] = result["compare"]["a"]
        finally:
            loader.close()
        if rank == 0:
            text = json.dumps(_jsonable(result), indent=1)
            if args.out:
                with open(args.out, "w") as f:
                    f.write(text + "\n")
            else:
                print(text, flush=True)
        return result
    finally:
        if started:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
