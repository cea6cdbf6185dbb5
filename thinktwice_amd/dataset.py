"""The host side of the reference's sample assembly, restated: which (route, frame) pairs are samples, what one frame's
measurement and supervision files become, the order samples are drawn in, and how the small targets of a batch are collated.
Host only: numpy and torch's CPU generator, no GPU, no kernel library loaded.  loader.DeviceBatchLoader joins these with the
device stages (png.py, labels.py, preprocess.py, sweeps.py).

Pinned to open_loop_training/code/datasets/carla_dataset.py (CarlaDataset.__init__ :28-90, offset_then_rotate :106-112,
get_data_info :115-203), datasets/samplers/group_sampler.py (:32-105) and datasets/samplers/distributed_sampler.py (:11-41) by
golden F22 (tests/golden/gen_f22_dataset.py runs the reference's own modules; tests/test_dataset_cpu.py compares every bit).

What the reference does, quirks included, and this module restates:
  * samples start at frame -history_query_index_lis[0] of a route and stop pred_len frames before its end (:54, :81); a route
    shorter than start + 1 + pred_len frames yields none (:75);
  * the per-town cap is compared with `>` BEFORE a route is added (:68, :72), so a town overshoots its cap by up to one route;
    towns are counted by the first six characters of their name (:63); with is_full the cap holds only for the validation
    towns, those with "02" or "05" in that prefix (:66);
  * is_local rewrites a route "../xyz" to "../dataset/xyz" (:78);
  * theta NaN -> 0, then - pi / 2 (:120-121); (x, y) -> (y, -x) (:123-124, :131-132, :148-149); future positions, the
    acceleration and the target point go through offset_then_rotate (:133, :141, :150); a command below 0 becomes 4, then
    1 is subtracted (:159-162); under `only_ap_brake` the first Beta parameters are replaced by 0.8 / 5.5, for the current
    frame and each future frame on its own (:178-180, :193-196).

Not restated: `_rand_another` (:236-243).  `__getitem__` calls it when prepare_train_data returns None, which happens only
when get_data_info returns None, and get_data_info never does: the path is dead in the reference.  A file that cannot be read
is an error here, as it is there.

[3P] unpinned.  mmcv is not installed where this was written, so no fixture pins how its `collate` stacks the small targets
CarlaCollect lists (configs/thinktwice.py:212-218).  The convention adopted -- torch's default_collate on what
CarlaFormatBundle leaves: arrays stacked along a new batch axis, lists collated element by element, float64 rounded to
float32 once -- lives in ONE place, `collate_targets`; the shapes are the ones synth.make_batch and synth.make_train_targets
define and the model reads."""
import io
import json
import math
import os
import pickle

import numpy as np
import torch

GRID_LEVELS = 6             # the Roach maps of one supervision file: `cnn_features`, a list of six arrays


# ------------------------------------------------------------------------------------------------------------ the index
class DatasetIndex:
    """CarlaDataset.__init__'s `data_infos` (carla_dataset.py:53-83): the list of (route_path, frame), in its order.

    route_lengths: the unpickled dataset_metadata.pkl, {town: {route: number of frames}}, or a path to that file.
    towns: cfg["train_town"] / cfg["val_town"].  cfg: a mapping with pred_len, history_query_index_lis, is_local,
    max_sample_per_town and, optionally, is_full.  root: the directory the route paths are relative to -- the reference's
    working directory; `path(route_path, ...)` joins it on.  `data_infos` holds the reference's own strings."""

    def __init__(self, route_lengths, towns, cfg, root=None):
        if isinstance(route_lengths, (str, bytes, os.PathLike)):
            with open(route_lengths, "rb") as f:
                route_lengths = pickle.load(f)
        self.cfg, self.root = cfg, root
        self.pred_len = cfg["pred_len"]
        self.history = list(cfg["history_query_index_lis"])
        self.is_local = bool(cfg["is_local"])
        self.is_full = bool(cfg["is_full"]) if "is_full" in cfg else False
        start = -self.history[0]                                                # :54
        cap = cfg["max_sample_per_town"]
        self.data_infos, self.town_counts = [], {}
        for town in towns:
            if town not in route_lengths:                                        # :60 no data collected
                continue
            name = town[:6]                                                      # :63
            self.town_counts.setdefault(name, 0)
            capped = not self.is_full or "02" in name or "05" in name            # :66-68
            if capped and self.town_counts[name] > cap[name]:
                continue
            for route, length in route_lengths[town].items():
                if capped and self.town_counts[name] > cap[name]:                # :72 checked before the route is added
                    break
                if length < start + 1 + self.pred_len:                           # :75
                    continue
                route_path = route[:3] + "dataset/" + route[3:] if self.is_local else route          # :78
                new = [(route_path, frame) for frame in range(start, length - self.pred_len)]         # :81
                self.data_infos += new
                self.town_counts[name] += len(new)

    def __len__(self):
        return len(self.data_infos)

    def __getitem__(self, i):
        return self.data_infos[i]

    def path(self, route_path, *more):
        return os.path.join(route_path if self.root is None else os.path.join(self.root, route_path), *more)


# ------------------------------------------------------------------------------------------------------------ one frame
def read_file(path):
    with open(path, "rb") as f:
        return f.read()


def offset_then_rotate(target, ref, yaw):
    """carla_dataset.py:106-112 in float64: (target - ref) in the frame turned by `yaw`, target [k, 2] -> [k, 2]."""
    final = target - ref
    R = np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
    return np.einsum("ij,kj->ki", R.T, final)


def frame_name(frame):
    return str(frame).zfill(4)


def frame_files(folder, frame, is_current, pred_len):
    """The files frame_info reads, in the order it reads them: (measurement JSONs, supervision .npy files)."""
    span = range(0, pred_len + 1) if is_current else range(0, 1)
    meas = [os.path.join(folder, "measurements", frame_name(frame + k) + ".json") for k in span]
    sup = [os.path.join(folder, "supervision", frame_name(frame + k) + ".npy") for k in span] if is_current else []
    return meas, sup


def _supervision(data, path):
    try:
        return np.load(io.BytesIO(data), allow_pickle=True).item()               # :99-104, .item() of :172
    except Exception as e:
        raise ValueError(f"{path}: not a supervision dictionary saved with np.save ({e})") from e


def frame_info(folder, frame, is_current, pred_len, read=read_file, name=None):
    """get_data_info (carla_dataset.py:115-203) for frame `frame` of the route at `folder`, in float64 as there: the same
    keys with the same values.  is_current: the key frame, which also reads the next pred_len measurement files and its own
    and the next pred_len supervision files; an older frame of the queue reads its one measurement file.
    read: path -> bytes; every file is read exactly once.  name: what scene_token and pts_filename are built from (the
    reference's route string), `folder` if None -- `folder` is where the files are read."""
    name = folder if name is None else name
    meas_files, sup_files = frame_files(folder, frame, is_current, pred_len)
    loaded = [json.loads(read(p)) for p in meas_files]
    m = loaded[0]
    res = {"scene_token": name, "frame_idx": frame}
    theta = m["theta"] if not np.isnan(m["theta"]) else 0                        # :120
    theta = theta - np.pi / 2                                                    # :121
    res["input_theta"] = theta
    res["input_x"] = m["y"]                                                      # :123-124
    res["input_y"] = -m["x"]
    ego_xy = np.stack([res["input_x"], res["input_y"]], axis=-1)
    if is_current:
        future = loaded[1:]
        fx = np.array([f["y"] for f in future])                                  # :131-132
        fy = -np.array([f["x"] for f in future])
        res["waypoints"] = offset_then_rotate(np.stack([fx, fy], axis=-1), ego_xy, theta)
        res["future_speed"] = [f["speed"] for f in future]
    res["speed"] = m["speed"]
    can_bus = np.zeros(18)
    can_bus[0], can_bus[1] = res["input_x"], res["input_y"]
    accel = np.array(m["acceleration"], dtype=np.float64)
    accel[:2] = offset_then_rotate(np.array(accel[:2])[np.newaxis, :], np.array([0, 0]), theta).squeeze(0)     # :141
    can_bus[7:10] = accel
    can_bus[10:13] = m["angular_velocity"]
    can_bus[13] = m["speed"]
    can_bus[-2] = theta
    can_bus[-1] = theta / np.pi * 180
    res["can_bus"] = can_bus
    res["target_point"] = offset_then_rotate(np.array([[m["y_target"], -m["x_target"]]]), ego_xy, theta).squeeze(0)   # :148-150
    res["target_point_aim"] = res["target_point"]
    command = m["target_command"]                                               # :159-167
    if command < 0:
        command = 4
    command -= 1
    if command not in (0, 1, 2, 3, 4, 5):
        raise ValueError(f"{meas_files[0]}: target_command {m['target_command']} is outside -1, 1..6")
    res["target_command_raw"] = torch.tensor(command).long()
    one_hot = [0] * 6
    one_hot[command] = 1
    res["target_command"] = torch.tensor(one_hot)
    res["pts_filename"] = os.path.join(name, "lidar", frame_name(frame) + ".npy")
    if is_current:
        sups = [_supervision(read(p), p) for p in sup_files]
        cur, future = sups[0], sups[1:]
        res["action"], res["action_mu"], res["action_sigma"] = cur["action"], cur["action_mu"], cur["action_sigma"]
        if cur["only_ap_brake"]:                                                 # :178-180
            res["action_mu"][0] = 0.8
            res["action_sigma"][0] = 5.5
        res["future_action_mu"] = [f["action_mu"] for f in future]
        res["future_action_sigma"] = [f["action_sigma"] for f in future]
        res["future_action"] = np.stack([f["action"] for f in future], axis=0)
        for k, f in enumerate(future):                                           # :193-196
            if f["only_ap_brake"]:
                res["future_action_mu"][k][0] = 0.8
                res["future_action_sigma"][k][0] = 5.5
        res["value"], res["feature"], res["grid_feature"] = cur["value"], cur["features"], cur["cnn_features"]
        res["future_feature"] = [f["features"] for f in future]
        res["future_value"] = [f["value"] for f in future]
        res["future_grid_feature"] = [f["cnn_features"] for f in future]
    return res


def load_cloud(data, name="<bytes>"):
    """The bytes of a lidar/NNNN.npy file -> its (n, 4) float32 array (x, y, z, intensity) as a read-only view of `data`:
    nothing is copied and nothing is unpickled.  ValueError, naming the file, for any other dtype or shape."""
    f = io.BytesIO(data)
    try:
        version = np.lib.format.read_magic(f)
        if version == (1, 0):
            shape, fortran, dtype = np.lib.format.read_array_header_1_0(f)
        elif version == (2, 0):
            shape, fortran, dtype = np.lib.format.read_array_header_2_0(f)
        else:
            raise ValueError(f"format version {version}")
    except ValueError as e:
        raise ValueError(f"{name}: not a .npy file ({e})") from e
    if dtype != np.dtype("<f4") or len(shape) != 2 or shape[1] != 4 or (fortran and shape[0] > 1):
        raise ValueError(f"{name}: a LiDAR sweep must be an (n, 4) float32 array in C order, the file holds {dtype} {shape}"
                         + (" in Fortran order" if fortran else ""))
    at, n = f.tell(), shape[0] * 4
    if len(data) - at < 4 * n:
        raise ValueError(f"{name}: {shape} float32 need {4 * n} bytes after the header, the file has {len(data) - at}")
    return np.frombuffer(data, dtype=np.float32, count=n, offset=at).reshape(shape[0], 4)


# ------------------------------------------------------------------------------------------------------------- samplers
class GroupSampler:
    """DistributedGroupSampler (group_sampler.py:32-105) over a dataset of `n` samples whose `flag` is all ones, as
    CarlaDataset sets it (carla_dataset.py:89): one group.  A seeded permutation, padded by repetition to a multiple of
    samples_per_gpu * world, cut into runs of samples_per_gpu that are permuted again, of which rank r takes the r-th
    stretch of num_samples."""

    def __init__(self, n, samples_per_gpu=1, world=1, rank=0, seed=0):
        if n < 1:
            raise ValueError("GroupSampler: the dataset is empty")
        if not 0 <= rank < world:
            raise ValueError(f"GroupSampler: rank {rank} of {world}")
        self.n, self.samples_per_gpu, self.world, self.rank = int(n), int(samples_per_gpu), int(world), int(rank)
        self.epoch = 0
        self.seed = seed if seed is not None else 0
        self.num_samples = int(math.ceil(self.n * 1.0 / self.samples_per_gpu / self.world)) * self.samples_per_gpu   # :56-58
        self.total_size = self.num_samples * self.world

    def __iter__(self):
        g = torch.Generator()
        g.manual_seed(self.epoch + self.seed)                                    # :63-64
        indice = np.arange(self.n)[list(torch.randperm(self.n, generator=g).numpy())].tolist()
        extra = self.total_size - len(indice)                                    # :73-81
        tmp = indice.copy()
        for _ in range(extra // self.n):
            indice.extend(tmp)
        indice.extend(tmp[:extra % self.n])
        spg = self.samples_per_gpu
        indices = [indice[j] for i in list(torch.randperm(len(indice) // spg, generator=g))           # :86-92
                   for j in range(i * spg, (i + 1) * spg)]
        offset = self.num_samples * self.rank                                    # :95-96
        return iter(indices[offset:offset + self.num_samples])

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch


class SequentialSampler:
    """DistributedSampler(shuffle=False) (distributed_sampler.py:11-41 over torch's class): the indices 0..n-1, repeated up
    to a multiple of `world`, of which rank r takes the r-th contiguous stretch."""

    def __init__(self, n, world=1, rank=0):
        if n < 1:
            raise ValueError("SequentialSampler: the dataset is empty")
        if not 0 <= rank < world:
            raise ValueError(f"SequentialSampler: rank {rank} of {world}")
        self.n, self.world, self.rank, self.epoch = int(n), int(world), int(rank), 0
        self.num_samples = math.ceil(self.n / self.world)
        self.total_size = self.num_samples * self.world

    def __iter__(self):
        indices = (list(range(self.n)) * math.ceil(self.total_size / self.n))[:self.total_size]        # :31-32
        per = self.total_size // self.world
        return iter(indices[self.rank * per:(self.rank + 1) * per])              # :36-38

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch


# -------------------------------------------------------------------------------------------------------------- collate
def _f32(values, shape=None):
    """The one float64 -> float32 rounding of the targets: np.float32(value), stacked along a new batch axis."""
    a = np.stack([np.asarray(v, dtype=np.float64) if shape is None else np.asarray(v, dtype=np.float64).reshape(shape)
                  for v in values]).astype(np.float32)
    return torch.from_numpy(a)


def collate_targets(infos):
    """frame_info(is_current=True) of the B samples of a batch -> the batch's small tensors, float32 on the host: the keys
    CarlaCollect lists (configs/thinktwice.py:212-218) except img, points, depth and seg, which the device stages build.

        waypoints [B, pred_len, 2]   target_point [B, 2]   target_command [B, 6]   target_command_raw [B] (int64)
        speed [B]   value [B]   feature [B, F]   action_mu, action_sigma [B, 2]
        grid_feature: 6 x [B, ...]   future_grid_feature: pred_len x 6 x [B, ...]
        future_action_mu, future_action_sigma: pred_len x [B, 2]   future_feature: pred_len x [B, F]
        future_speed, future_value: pred_len x [B]

    The single owner of the collate convention ([3P] unpinned, see the module docstring) and of the float64 -> float32
    rounding: every value is np.float32 of frame_info's."""
    if not infos:
        raise ValueError("collate_targets: no samples")
    P = len(infos[0]["future_speed"])
    col = lambda k, shape=None: _f32([i[k] for i in infos], shape)              # noqa: E731
    each = lambda k, j, shape=None: _f32([i[k][j] for i in infos], shape)       # noqa: E731
    out = {
        "waypoints": col("waypoints"), "target_point": col("target_point"),
        "target_command": _f32([i["target_command"].numpy() for i in infos]),
        "target_command_raw": torch.stack([i["target_command_raw"] for i in infos]),
        "speed": col("speed", ()), "value": col("value", ()), "feature": col("feature"),
        "action_mu": col("action_mu"), "action_sigma": col("action_sigma"),
        "grid_feature": [each("grid_feature", j) for j in range(len(infos[0]["grid_feature"]))],
        "future_grid_feature": [[_f32([i["future_grid_feature"][p][j] for i in infos])
                                 for j in range(len(infos[0]["future_grid_feature"][p]))] for p in range(P)],
        "future_action_mu": [each("future_action_mu", p) for p in range(P)],
        "future_action_sigma": [each("future_action_sigma", p) for p in range(P)],
        "future_feature": [each("future_feature", p) for p in range(P)],
        "future_speed": [each("future_speed", p, ()) for p in range(P)],
        "future_value": [each("future_value", p, ()) for p in range(P)],
    }
    return out
