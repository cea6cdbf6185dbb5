"""From a dataset directory to `forward_train` batches that live on the device: the reference's CarlaDataset +
DistributedGroupSampler + collate (open_loop_training/code/datasets/carla_dataset.py:205-234, configs/thinktwice.py:204-279)
joined to the device stages of this package, which run on a side stream while the previous step trains.

    index = dataset.DatasetIndex("dataset_metadata.pkl", cfg["train_town"], cfg, root=workdir)
    loader = DeviceBatchLoader(index, cfg, ida_aug_conf, batch_size=8, seed=0, rank=rank, world=world)
    for epoch in range(epochs):
        loader.set_epoch(epoch)
        for batch in loader:                # device-resident forward_train batch; img_metas on the host
            trainer.step(batch)             # or model.train_step(batch, optimizer) on the autograd route

How one batch is built:
  1. reader threads (a ThreadPoolExecutor; they never touch the GPU) read the files of every sample -- T x N camera PNGs,
     N depth and N seg PNGs of the KEY frame, T LiDAR .npy files, 1 + pred_len + (T - 1) measurement JSONs, 1 + pred_len
     supervision files -- and run dataset.frame_info on them.  The reference also loads the older frames' depth and seg
     files and throws them away (union2one keeps queue[-1]'s); skipping those reads is deliberate;
  2. the coordinating thread -- the one that iterates the loader -- draws everything random, in sample order: the
     IdaSampler parameters and the PhotometricSampler programs.  What a batch holds therefore does not depend on thread
     timing or on `threads`;
  3. on the loader's one side stream it then launches PngDecoder.decode_sample_batch(check=False), RawLabelDecoder,
     TrainImagePipeline(params=, augment=), SweepUnion and the upload of the collated targets: ONE pinned blob, one
     host-to-device copy, the batch's small tensors being views of the device copy.  Every in-flight slot owns its decoder,
     pipeline and pinned blob; a blob is refilled only after the event behind its copy has completed;
  4. an event closes the batch.  `__next__` waits for it on the host -- the one host synchronisation of a batch --, reads the
     PNG statuses from their pinned copy (PngDecodeError naming the file paths if one is not zero), lets the consumer's
     current stream wait on it, marks every device tensor with record_stream(consumer stream), and assembles the batch with
     preprocess.fill_batch and sweeps.fill_sweeps; the remaining per-sweep meta keys come from calib as
     synth.make_img_metas sets them, plus scene_token, frame_idx, img_filename and pts_filename.
With prefetch = p the stages of the next p batches are already queued when a batch is handed over, and the files of one
more are being read.  prefetch = 0 builds every batch when it is asked for.

Errors.  A missing or unreadable file raises from the `__next__` of the batch that needed it, the message naming the path; a
corrupt PNG raises PngDecodeError there.  Nothing is retried: the reference's `_rand_another` path is dead code
(get_data_info never returns None, see dataset.py) and is not restated.  After an error, after close() and on leaving the
context manager no reader thread is alive and the side stream is idle.  Nothing here forks or spawns."""
import collections
import concurrent.futures
import os
import time
import warnings

import numpy as np
import torch

from . import calib, dataset, labels, photometric, preprocess, sweeps
from . import png as png_mod

MAX_THREADS = 16


def eval_ida_params(ida_aug_conf):
    """sample_ida_augmentation's evaluation branch (transform.py:264-272) as the IdaParams every camera gets when
    train=False; preprocess.ida_mat of it equals calib.eval_ida_mat(final_dim)."""
    c = ida_aug_conf
    H, W = c["H"], c["W"]
    fH, fW = c["final_dim"]
    resize = max(fH / H, fW / W)
    newW, newH = int(W * resize), int(H * resize)
    crop_h = int((1 - np.mean(c["bot_pct_lim"])) * newH) - fH
    crop_w = int(max(0, newW - fW) / 2)
    return preprocess.IdaParams(float(resize), newH, newW, crop_h, crop_w, False)


def sample_files(folder, frame, history, cameras):
    """The image and LiDAR files of one sample: (rgb [T][N], depth [N], seg [N], lidar [T]) paths, oldest frame first; the
    labels are the key frame's (loading.py:46, :85, :133)."""
    name = dataset.frame_name
    rgb = [[os.path.join(folder, cam, name(frame + h) + ".png") for cam in cameras] for h in history]
    dep = [os.path.join(folder, cam.replace("rgb", "depth"), name(frame) + ".png") for cam in cameras]
    seg = [os.path.join(folder, cam.replace("rgb", "seg"), name(frame) + ".png") for cam in cameras]
    lidar = [os.path.join(folder, "lidar", name(frame + h) + ".npy") for h in history]
    return rgb, dep, seg, lidar


def read_sample(folder, route_path, frame, history, cameras, pred_len, read=dataset.read_file):
    """Everything one sample needs from the disk, read once each (a reader thread's job; no GPU): the file bytes, the
    parsed clouds and frame_info of every frame of the queue, the key frame's with is_current=True."""
    if history[-1] != 0:
        raise ValueError(f"history_query_index_lis must end in 0 (the key frame), got {history}")
    rgb, dep, seg, lidar = sample_files(folder, frame, history, cameras)
    t0 = time.perf_counter()
    out = {"route": route_path, "frame": frame,
           "rgb_paths": rgb, "depth_paths": dep, "seg_paths": seg, "lidar_paths": lidar,
           "rgb": [[read(p) for p in per] for per in rgb], "depth": [read(p) for p in dep], "seg": [read(p) for p in seg],
           "clouds": [dataset.load_cloud(read(p), p) for p in lidar],
           "infos": [dataset.frame_info(folder, frame + h, h == 0, pred_len, read, name=route_path) for h in history]}
    out["seconds"] = time.perf_counter() - t0
    return out


def _rng_state(rng):
    name, keys, pos, has_gauss, cached = rng.get_state()
    return {"name": name, "keys": [int(k) for k in keys], "pos": int(pos), "has_gauss": int(has_gauss), "cached": float(cached)}


def _load_rng(rng, s):
    rng.set_state((s["name"], np.asarray(s["keys"], dtype=np.uint32), s["pos"], s["has_gauss"], s["cached"]))


def sampler_state(ida_sampler, photometric_sampler):
    """The random streams of a training loader as plain Python data (a checkpoint's meta): the IdaSampler's RandomState, the
    PhotometricSampler's RandomState and its `reads` (the sample count its schedule runs on).  None for a sampler that is off."""
    return {"ida": None if ida_sampler is None else _rng_state(ida_sampler.rng),
            "photometric": None if photometric_sampler is None else {"rng": _rng_state(photometric_sampler.rng),
                                                                     "reads": int(photometric_sampler.reads)}}


def load_sampler_state(ida_sampler, photometric_sampler, s):
    for name, have, saved in (("ida", ida_sampler, s["ida"]), ("photometric", photometric_sampler, s["photometric"])):
        if (have is None) != (saved is None):
            raise ValueError(f"load_sampler_state: the {name} sampler is {'off' if have is None else 'on'} here and "
                             f"{'off' if saved is None else 'on'} in the saved state")
    if ida_sampler is not None:
        _load_rng(ida_sampler.rng, s["ida"])
    if photometric_sampler is not None:
        _load_rng(photometric_sampler.rng, s["photometric"]["rng"])
        photometric_sampler.reads = int(s["photometric"]["reads"])


class _Slot:
    """What one in-flight batch owns: its decoder and pipeline objects, its pinned target blob and the event behind the
    blob's last copy."""

    def __init__(self, loader):
        self.png = png_mod.PngDecoder(device=loader.device, **loader.png_args)
        self.pipeline = preprocess.TrainImagePipeline(loader.ida_aug_conf, undistort=loader.undistort, device=loader.device)
        self.blob = self.status_host = self.copied = None


class DeviceBatchLoader:
    """See the module text.  index: a dataset.DatasetIndex.  cfg: a mapping with camera_names and seg_label_idxs; pred_len
    and history_query_index_lis are the index's.  png: the keyword arguments of every slot's PngDecoder.  augment: True for
    ImageTransformMulti(aug=True)'s colour augmentation (training only).  read: path -> bytes, called from reader threads.
    `last` describes the batch handed over most recently: samples [(route, frame)], params, programs (None without
    augmentation), files (the PNG paths in the decoder's order) and timings."""

    def __init__(self, index, cfg, ida_aug_conf, batch_size=8, device="cuda", train=True, seed=0, rank=0, world=1, prefetch=2,
                 threads=8, png=None, augment=True, read=dataset.read_file, undistort=True, pad_to=None):
        if not 1 <= int(threads) <= MAX_THREADS:
            raise ValueError(f"threads must be 1..{MAX_THREADS}, got {threads}")
        if int(prefetch) < 0 or int(batch_size) < 1:
            raise ValueError(f"prefetch {prefetch} must be >= 0 and batch_size {batch_size} >= 1")
        self.index, self.cfg, self.ida_aug_conf = index, cfg, dict(ida_aug_conf)
        self.batch_size, self.train, self.seed, self.rank, self.world = int(batch_size), bool(train), seed, int(rank), int(world)
        self.prefetch, self.threads, self.read, self.undistort = int(prefetch), int(threads), read, undistort
        self.png_args = dict(verify=("adler32",), segments="auto") if png is None else dict(png)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("DeviceBatchLoader needs a GPU device: the stages have no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.cameras = list(cfg["camera_names"])
        self.history, self.pred_len = list(index.history), index.pred_len
        self.final_dim = tuple(self.ida_aug_conf["final_dim"])
        if len(index) == 0:
            raise ValueError("the dataset index is empty")
        self.sampler = (dataset.GroupSampler(len(index), self.batch_size, self.world, self.rank, seed) if self.train
                        else dataset.SequentialSampler(len(index), self.world, self.rank))
        rs = lambda k: np.random.RandomState([int(seed or 0), self.rank, k])    # noqa: E731
        self.ida_sampler = preprocess.IdaSampler(self.ida_aug_conf, rs(0)) if self.train else None
        self.augment = photometric.PhotometricSampler(self.batch_size, rs(1)) if (augment and self.train) else None
        self.label_decoder = labels.RawLabelDecoder(cfg["seg_label_idxs"])
        self.union = sweeps.SweepUnion(device=self.device, pad_to=pad_to)
        intr, l2c, l2i = calib.camera_tables()
        if len(self.cameras) != len(l2c):
            raise ValueError(f"{len(self.cameras)} cameras, the calibration tables hold {len(l2c)}")
        self._calib = (intr, l2c, l2i)
        self.stream = torch.cuda.Stream(self.device)
        self._slots = [_Slot(self) for _ in range(self.prefetch + 1)]
        self.stream.wait_stream(torch.cuda.current_stream(self.device))          # (the slots' undistortion maps went up there)
        self._pool = None
        self._batches = collections.OrderedDict()          # number -> record of every batch read, launched or failed
        self._plan, self._next, self._read_to, self._launch_to, self._failed = [], 0, 0, 0, False
        self.last = None

    # ------------------------------------------------------------------------------------------------------ iteration
    def set_epoch(self, epoch):
        self.sampler.set_epoch(epoch)

    def __len__(self):
        return -(-len(self.sampler) // self.batch_size)

    def state(self):
        """What a bit-identical resume needs of this loader BETWEEN epochs (sampler_state: the augmentation streams; the
        sample order is a function of seed and epoch).  RuntimeError while an epoch is being iterated: the draws of the
        prefetched batches are already taken."""
        if self._pool is not None:
            raise RuntimeError("DeviceBatchLoader.state(): an epoch is being iterated; the state is defined between epochs")
        return sampler_state(self.ida_sampler, self.augment)

    def load_state(self, s):
        if self._pool is not None:
            raise RuntimeError("DeviceBatchLoader.load_state(): an epoch is being iterated; the state is defined between epochs")
        load_sampler_state(self.ida_sampler, self.augment, s)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __iter__(self):
        self.close()
        order = list(self.sampler)
        self._plan = [order[i:i + self.batch_size] for i in range(0, len(order), self.batch_size)]
        self._next = self._read_to = self._launch_to = 0
        self._failed = False
        self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="tt-loader-read")
        return self

    def close(self):
        """Stop: no reader thread stays alive, the side stream is idle, nothing launched is kept."""
        if self._pool is not None:
            self._pool.shutdown(wait=True, cancel_futures=True)
            self._pool = None
        self.stream.synchronize()
        self._batches.clear()
        self._plan = []

    def _submit(self, k):
        samples = [self.index[i] for i in self._plan[k]]
        futures = [self._pool.submit(read_sample, self.index.path(route), route, frame, self.history, self.cameras,
                                     self.pred_len, self.read) for route, frame in samples]
        self._batches[k] = {"samples": samples, "futures": futures, "error": None, "submitted": time.perf_counter()}

    def __next__(self):
        k = self._next
        if self._pool is None or k >= len(self._plan):
            self.close()
            raise StopIteration
        ahead = self.prefetch + (1 if self.prefetch else 0)
        while self._read_to < min(len(self._plan), k + ahead + 1):
            self._submit(self._read_to)
            self._read_to += 1
        while self._launch_to < min(len(self._plan), k + self.prefetch + 1) and not self._failed:
            rec = self._batches[self._launch_to]
            try:
                self._launch(self._launch_to, rec)
            except Exception as e:                          # raised from the __next__ of the batch that needed the file
                rec["error"], self._failed = e, True
            self._launch_to += 1
        rec = self._batches.pop(k)
        self._next += 1
        if rec["error"] is not None:
            self.close()
            raise rec["error"]
        try:
            return self._hand_over(rec)
        except Exception:
            self.close()
            raise

    # --------------------------------------------------------------------------------------------------- one batch
    def _launch(self, k, rec):
        """Queue batch k's device stages on the side stream (coordinating thread)."""
        t0 = time.perf_counter()
        read = [f.result() for f in rec["futures"]]
        t1 = time.perf_counter()
        rec["futures"] = None
        B, T, N = len(read), len(self.history), len(self.cameras)
        if self.train:
            params = self.ida_sampler.sample(B, N)
        else:
            params = [[eval_ida_params(self.ida_aug_conf)] * N for _ in range(B)]
        preprocess.check_ida_params(params, self.final_dim)
        fh, fw = self.final_dim
        programs = self.augment.programs(B, fh, fw) if self.augment is not None else None
        infos = [r["infos"] for r in read]
        targets = dataset.collate_targets([i[-1] for i in infos])
        can_bus = [[i["can_bus"] for i in per] for per in infos]
        with warnings.catch_warnings():                     # (the clouds are read-only views of the file bytes)
            warnings.simplefilter("ignore", UserWarning)
            clouds = [[torch.from_numpy(c) for c in r["clouds"]] for r in read]
        slot = self._slots[k % len(self._slots)]
        rec["files"] = ([p for r in read for per in r["rgb_paths"] for p in per] + [p for r in read for p in r["depth_paths"]]
                        + [p for r in read for p in r["seg_paths"]])
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            begin = torch.cuda.Event(enable_timing=True)
            begin.record(self.stream)
            host = [time.perf_counter()]                    # the coordinating thread's time in each stage's call
            raw, depth_png, seg_png, status = slot.png.decode_sample_batch([r["rgb"] for r in read], [r["depth"] for r in read],
                                                                           [r["seg"] for r in read], check=False)
            if slot.status_host is None or slot.status_host.numel() < status.numel():
                slot.status_host = torch.empty(max(status.numel(), 64), dtype=torch.int32, pin_memory=True)
            slot.status_host[:status.numel()].copy_(status, non_blocking=True)
            host.append(time.perf_counter())
            depth, seg = self.label_decoder(raw, depth_png, seg_png)
            host.append(time.perf_counter())
            out = slot.pipeline(raw, depth, seg, params=params, augment=programs, pinned_programs=True)
            host.append(time.perf_counter())
            cloud = self.union(clouds, can_bus)
            host.append(time.perf_counter())
            small = self._upload(slot, targets)
            host.append(time.perf_counter())
            done = torch.cuda.Event(enable_timing=True)
            done.record(self.stream)
        rec.update(begin=begin, out=out, cloud=cloud, small=small, done=done, status=slot.status_host[:status.numel()], infos=infos,
                   params=params, programs=programs,
                   timings={"host_stage_s": dict(zip(("png", "labels", "pipeline", "union", "targets"), np.diff(host).tolist())),
                            "read_wait_s": t1 - t0, "read_s": max(r["seconds"] for r in read), "launch_s": time.perf_counter() - t1,
                            "png_packed_bytes": slot.png.last_packed_bytes,
                            "cloud_bytes": sum(c.numel() * 4 for per in clouds for c in per)})

    def _upload(self, slot, targets):
        """The collated targets as one pinned blob and one copy; returns the same nest with views of the device blob."""
        flat = []

        def walk(v):
            if isinstance(v, list):
                return [walk(x) for x in v]
            flat.append(v)
            return len(flat) - 1

        nest = {k: walk(v) for k, v in targets.items()}
        offsets, at = [], 0
        for t in flat:
            offsets.append(at)
            at += -(-t.numel() * t.element_size() // 16) * 16
        if slot.copied is not None:
            slot.copied.synchronize()                       # the blob's last copy has left it
        if slot.blob is None or slot.blob.numel() < at:
            slot.blob = torch.empty(at, dtype=torch.uint8, pin_memory=True)
        for t, o in zip(flat, offsets):
            n = t.numel() * t.element_size()
            slot.blob[o:o + n] = t.contiguous().view(-1).view(torch.uint8)
        dev = torch.empty(at, dtype=torch.uint8, device=self.device)
        dev.copy_(slot.blob[:at], non_blocking=True)
        slot.copied = torch.cuda.Event()
        slot.copied.record(self.stream)
        views = [dev[o:o + t.numel() * t.element_size()].view(t.dtype).view(t.shape) for t, o in zip(flat, offsets)]

        def back(v):
            return [back(x) for x in v] if isinstance(v, list) else views[v]

        out = {k: back(v) for k, v in nest.items()}
        out["_blob"], out["_blob_bytes"] = dev, at
        return out

    def _metas(self, rec):
        intr, l2c, l2i = self._calib
        metas = []
        for infos in rec["infos"]:
            per_sweep = []
            for t, info in enumerate(infos):
                per_sweep.append({"cam_intrinsic": torch.from_numpy(intr.copy()), "lidar2cam": torch.from_numpy(l2c.copy()),
                                  "lidar2img": torch.from_numpy(l2i.copy()), "scene_token": info["scene_token"],
                                  "frame_idx": info["frame_idx"], "pts_filename": info["pts_filename"],
                                  "img_filename": [os.path.join(info["scene_token"], cam, dataset.frame_name(info["frame_idx"]) + ".png")
                                                   for cam in self.cameras]})
            metas.append(per_sweep)
        return metas

    def _hand_over(self, rec):
        t0 = time.perf_counter()
        rec["done"].synchronize()                           # the batch's one host synchronisation
        waited = time.perf_counter() - t0
        failed = [(rec["files"][i], png_mod.STATUS_NAMES.get(s, str(s))) for i, s in enumerate(rec["status"].tolist()) if s != 0]
        if failed:
            raise png_mod.PngDecodeError(failed)
        consumer = torch.cuda.current_stream(self.device)
        consumer.wait_event(rec["done"])
        out, cloud, small = rec["out"], rec["cloud"], rec["small"]
        for t in (out["img"], out["depth"], out["seg"], cloud["points"], small.pop("_blob")):
            t.record_stream(consumer)
        rec["timings"]["target_bytes"] = small.pop("_blob_bytes")
        rec["timings"]["device_ms"] = rec["begin"].elapsed_time(rec["done"])    # first launch to last, on the side stream
        T, N = len(self.history), len(self.cameras)
        l2c = np.broadcast_to(self._calib[1], (T, N, 4, 4))
        batch = {"img_metas": self._metas(rec)}
        preprocess.fill_batch(batch, out)
        sweeps.fill_sweeps(batch, cloud, [sweeps.sweep_metas(np.stack([i["can_bus"] for i in per]), l2c, ps)
                                          for per, ps in zip(rec["infos"], cloud["points_size"])])
        batch.update(small)
        rec["timings"]["event_wait_s"] = waited
        self.last = {"samples": rec["samples"], "params": rec["params"], "programs": rec["programs"], "files": rec["files"],
                     "timings": rec["timings"]}
        return batch
