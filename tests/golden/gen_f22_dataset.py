"""Golden F22: the reference's own sample assembly on the host -- CarlaDataset.__init__'s `data_infos` and get_data_info
(open_loop_training/code/datasets/carla_dataset.py:28-90, :115-203), DistributedGroupSampler (datasets/samplers/
group_sampler.py) and DistributedSampler(shuffle=False) (datasets/samplers/distributed_sampler.py) -- run from the reference's
own modules on a few tiny seeded routes.

    python tests/golden/gen_f22_dataset.py            writes tests/golden/f22_dataset.npz
    python tests/golden/gen_f22_dataset.py --check    regenerates and compares with the committed file bit for bit

Build container only (needs the reference checkout that ref_stubs.py names).  Recipe of gen_f20_sweep_union.py: the modules
are imported from where they lie, under synthetic parent packages so that datasets/__init__.py does not run; their
third-party imports are the stand-ins of ref_stubs.py plus the few set below.  What is NOT the reference's:
  * mmdet3d's Compose is an identity stand-in (the pipelines are not what is pinned), mmcv's Registry a no-op one,
    mmcv.runner.get_dist_info returns (0, 1) -- every sampler here gets its rank and world explicitly;
  * CarlaDataset.__init__ opens ../dataset/dataset_metadata.pkl relative to the working directory: the script lays out a
    temporary directory accordingly (dataset/dataset_metadata.pkl, the routes under dataset/, work/ as the working directory)
    and runs it from work/.
The routes' supervision arrays are tiny (features of 8 values, six Roach maps of a few values): get_data_info does not look
at their shapes.  The file holds data only: the seeded inputs (`write_routes` rebuilds the files from them) and what the
reference returned."""
import importlib.util
import json
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_stubs  # noqa: E402

NAME = "f22_dataset.npz"
SEED = 22
PRED_LEN = 4
FEATURES = 8
GRID_SHAPES = [(1,), (1,), (2, 3, 3), (2, 2, 2), (2, 1, 1), (1, 1, 1)]
# the routes that have files: (town, route key as dataset_metadata.pkl holds it, frames)
ROUTES = [("town01_00", "../town01_00/routes_r0", 9), ("town01_00", "../town01_00/routes_r2", 10)]
NAN_THETA = {(0, 1), (1, 4), (0, 7)}                # (route, frame)
VOID_COMMAND = {(0, 1), (1, 3), (1, 4)}             # target_command = -1
AP_BRAKE = {(0, 1), (0, 3), (0, 5), (1, 6), (1, 9)}
# get_data_info calls: (route, frame, is_current)
INFO_CASES = [(0, 1, True), (0, 0, False), (0, 4, True), (1, 5, True), (1, 4, False)]
# data_infos: the metadata dictionary and the configurations it is indexed under
METADATA = {
    "town01_00": {"../town01_00/routes_r0": 9, "../town01_00/routes_r1": 5, "../town01_00/routes_r2": 10,
                  "../town01_00/routes_r3": 8},                                  # r1 too short; the cap is passed after r2
    "town01_01": {"../town01_01/routes_r4": 8},                                  # town01 is over its cap: skipped unless is_full
    "town02_val": {"../town02_val/routes_r5": 9, "../town02_val/routes_r6": 9, "../town02_val/routes_r7": 12},
    "town06_00": {"../town06_00/routes_r8": 6, "../town06_00/routes_r9": 7},
}
TOWNS = ["town01_00", "town01_01", "town03_00", "town02_val", "town06_00"]       # town03_00: not in the dictionary
CAPS = {"town01": 5, "town02": 3, "town03": 100, "town06": 100}
INDEX_CASES = [dict(is_full=False, history=[-1, 0]), dict(is_full=True, history=[-1, 0]), dict(is_full=False, history=[-3, -1, 0]),
               dict(is_full=None, history=[-2, 0])]                              # None: the key is absent from cfg
# (n, samples_per_gpu, world, rank, epoch, seed)
GROUP_CASES = [(17, 2, 1, 0, 0, 0), (17, 2, 2, 0, 3, 0), (17, 2, 2, 1, 3, 0), (16, 8, 2, 1, 1, 5), (5, 8, 1, 0, 0, 7),
               (3, 2, 4, 2, 2, 1), (23, 3, 2, 1, 0, None)]
SEQ_CASES = [(17, 1, 0), (17, 2, 0), (17, 2, 1), (16, 4, 3), (3, 4, 2), (2, 5, 4)]     # (n, world, rank)
MEAS_COLUMNS = ["x", "y", "theta", "speed", "x_target", "y_target", "target_command", "ax", "ay", "az", "wx", "wy", "wz"]


# ------------------------------------------------------------------------------------- inputs (no reference needed below)
def make_routes():
    """The seeded inputs: {r{k}_meas [L, 13] f64, r{k}_action [L, 3], r{k}_action_mu / _action_sigma [L, 2], r{k}_value [L],
    r{k}_features [L, 8], r{k}_cnn [L, 40] (all f32; the six Roach maps of GRID_SHAPES, flattened, one after the other),
    r{k}_only_ap_brake [L] bool}."""
    rng = np.random.default_rng(SEED)
    out = {}
    for k, (_, _, L) in enumerate(ROUTES):
        meas = np.empty((L, len(MEAS_COLUMNS)))
        meas[:, 0:2] = rng.uniform(-300, 300, 2) + np.cumsum(rng.uniform(-2, 2, (L, 2)), axis=0)
        meas[:, 2] = rng.uniform(-np.pi, np.pi) + np.cumsum(rng.uniform(-0.2, 0.2, L))
        meas[:, 3] = rng.uniform(0, 9, L)
        meas[:, 4:6] = meas[:, 0:2] + rng.uniform(-40, 40, (L, 2))
        meas[:, 6] = rng.integers(1, 7, L)
        meas[:, 7:13] = rng.normal(size=(L, 6))
        for f in range(L):
            if (k, f) in NAN_THETA:
                meas[f, 2] = np.nan
            if (k, f) in VOID_COMMAND:
                meas[f, 6] = -1
        out[f"r{k}_meas"] = meas
        out[f"r{k}_action"] = rng.uniform(-1, 1, (L, 3)).astype(np.float32)
        out[f"r{k}_action_mu"] = rng.uniform(0.2, 4, (L, 2)).astype(np.float32)
        out[f"r{k}_action_sigma"] = rng.uniform(0.2, 4, (L, 2)).astype(np.float32)
        out[f"r{k}_value"] = rng.normal(size=L).astype(np.float32)
        out[f"r{k}_features"] = rng.normal(size=(L, FEATURES)).astype(np.float32)
        out[f"r{k}_cnn"] = rng.normal(size=(L, sum(int(np.prod(s)) for s in GRID_SHAPES))).astype(np.float32)
        out[f"r{k}_only_ap_brake"] = np.array([(k, f) in AP_BRAKE for f in range(L)])
    return out


def measurement_json(row):
    """One measurements/NNNN.json from a row of r{k}_meas: Python's json writes a float64 so that it reads back bit for bit,
    and NaN as the token NaN, as the dataset's recorder did."""
    v = dict(zip(MEAS_COLUMNS, (float(x) for x in row)))
    return json.dumps({"x": v["x"], "y": v["y"], "theta": v["theta"], "speed": v["speed"], "x_target": v["x_target"],
                       "y_target": v["y_target"], "target_command": int(v["target_command"]),
                       "acceleration": [v["ax"], v["ay"], v["az"]], "angular_velocity": [v["wx"], v["wy"], v["wz"]]})


def split_levels(flat):
    """[40] -> the six arrays of GRID_SHAPES (copies)."""
    at = np.cumsum([0] + [int(np.prod(s)) for s in GRID_SHAPES])
    return [flat[at[j]:at[j + 1]].reshape(s).copy() for j, s in enumerate(GRID_SHAPES)]


def supervision_dict(arrays, k, f):
    return {"action": arrays[f"r{k}_action"][f].copy(), "action_mu": arrays[f"r{k}_action_mu"][f].copy(),
            "action_sigma": arrays[f"r{k}_action_sigma"][f].copy(), "only_ap_brake": bool(arrays[f"r{k}_only_ap_brake"][f]),
            "value": arrays[f"r{k}_value"][f].copy(), "features": arrays[f"r{k}_features"][f].copy(),
            "cnn_features": split_levels(arrays[f"r{k}_cnn"][f])}


def write_routes(dataset_dir, arrays):
    """The routes' measurements/ and supervision/ files under `dataset_dir` from the input arrays -> [route directory]."""
    dirs = []
    for k, (_, route, L) in enumerate(ROUTES):
        d = os.path.join(dataset_dir, route[3:])
        os.makedirs(os.path.join(d, "measurements"))
        os.makedirs(os.path.join(d, "supervision"))
        for f in range(L):
            with open(os.path.join(d, "measurements", f"{f:04d}.json"), "w") as fh:
                fh.write(measurement_json(arrays[f"r{k}_meas"][f]))
            np.save(os.path.join(d, "supervision", f"{f:04d}.npy"), np.array(supervision_dict(arrays, k, f), dtype=object),
                    allow_pickle=True)
        dirs.append(d)
    return dirs


def flatten_info(res, prefix):
    """A get_data_info result as named arrays (every value, dtype kept).  The Roach maps of `grid_feature` are checked
    against GRID_SHAPES and stored flattened, one after the other (future_grid_feature: one such row per future frame)."""
    out = {}
    for key, v in res.items():
        if key in ("grid_feature", "future_grid_feature"):
            nest = [v] if key == "grid_feature" else v
            assert all([np.asarray(a).shape for a in level] == GRID_SHAPES for level in nest)
            rows = np.stack([np.concatenate([np.asarray(a).ravel() for a in level]) for level in nest])
            out[prefix + key] = rows[0] if key == "grid_feature" else rows
        elif isinstance(v, str):
            out[prefix + key] = np.array(v)
        elif hasattr(v, "numpy"):
            out[prefix + key] = v.numpy()
        elif isinstance(v, list):
            out[prefix + key] = np.stack([np.asarray(a) for a in v])
        else:
            out[prefix + key] = np.asarray(v)
    return out


def index_cfg(case):
    cfg = {"pred_len": PRED_LEN, "history_query_index_lis": case["history"], "is_local": True, "max_sample_per_town": CAPS}
    if case["is_full"] is not None:
        cfg["is_full"] = case["is_full"]
    return cfg


# ------------------------------------------------------------------------------------------------------- the reference
def _load(pkg, rel, name):
    path = os.path.join(ref_stubs.OLT, "code", *rel, name + ".py")
    spec = importlib.util.spec_from_file_location(f"{pkg}.{name}", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def _load_reference():
    ref_stubs.install()
    for name in ("matplotlib", "matplotlib.pyplot", "mmcv.parallel", "mmdet.datasets", "mmdet3d.datasets",
                 "mmdet3d.datasets.pipelines", "PIL", "PIL.Image", "nuscenes", "nuscenes.eval", "nuscenes.eval.common",
                 "nuscenes.eval.common.utils", "mmcv.utils.registry"):
        if name not in sys.modules:
            ref_stubs._mod(name)
    sys.modules["mmdet.datasets"].DATASETS = ref_stubs._Registry("datasets")
    sys.modules["mmdet.datasets"].CustomDataset = object
    sys.modules["mmdet3d.datasets.pipelines"].Compose = lambda pipeline: (lambda x: x)
    sys.modules["mmcv.utils.registry"].Registry = ref_stubs._Registry
    sys.modules["mmcv.runner"].get_dist_info = lambda: (0, 1)
    for sub, rel in (("datasets", ("datasets",)), ("datasets.samplers", ("datasets", "samplers"))):
        pkg = types.ModuleType(f"{ref_stubs.REF_PKG}.{sub}")                    # (the packages' __init__.py import the builders)
        pkg.__path__ = [os.path.join(ref_stubs.OLT, "code", *rel)]
        sys.modules[pkg.__name__] = pkg
    cd = _load(f"{ref_stubs.REF_PKG}.datasets", ("datasets",), "carla_dataset")
    gs = _load(f"{ref_stubs.REF_PKG}.datasets.samplers", ("datasets", "samplers"), "group_sampler")
    ds = _load(f"{ref_stubs.REF_PKG}.datasets.samplers", ("datasets", "samplers"), "distributed_sampler")
    return cd, gs, ds


class _Flagged:
    def __init__(self, n):
        self.flag = np.ones(n, dtype=np.uint8)                                  # carla_dataset.py:89

    def __len__(self):
        return len(self.flag)


def generate():
    cd, gs, ds = _load_reference()
    arrays = dict(seed=np.array([SEED]), pred_len=np.array([PRED_LEN]))
    arrays.update(make_routes())
    arrays["routes"] = np.array([r for _, r, _ in ROUTES])
    arrays["info_cases"] = np.array([[r, f, int(c)] for r, f, c in INFO_CASES])
    arrays["index_metadata"] = np.array(json.dumps(METADATA))
    arrays["index_towns"] = np.array(TOWNS)
    arrays["index_caps"] = np.array(json.dumps(CAPS))
    arrays["index_cases"] = np.array(json.dumps(INDEX_CASES))
    arrays["group_cases"] = np.array([[n, s, w, r, e, -1 if seed is None else seed] for n, s, w, r, e, seed in GROUP_CASES])
    arrays["seq_cases"] = np.array(SEQ_CASES)
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "dataset"))
        os.makedirs(os.path.join(tmp, "work"))
        write_routes(os.path.join(tmp, "dataset"), arrays)
        os.chdir(os.path.join(tmp, "work"))
        try:
            for c, case in enumerate(INDEX_CASES):
                with open(os.path.join(tmp, "dataset", "dataset_metadata.pkl"), "wb") as f:
                    pickle.dump(METADATA, f)
                data = cd.CarlaDataset(index_cfg(case), TOWNS, [], True, [])
                assert len(data.flag) == len(data.data_infos)
                arrays[f"index{c}_routes"] = np.array([r for r, _ in data.data_infos])
                arrays[f"index{c}_frames"] = np.array([f for _, f in data.data_infos])
            for c, (r, frame, current) in enumerate(INFO_CASES):                  # `data`: pred_len 4, is_local
                folder = [p for p, _ in data.data_infos if p.endswith(ROUTES[r][1][3:])][0]
                arrays.update(flatten_info(data.get_data_info(folder, frame, is_current=current), f"info{c}_"))
        finally:
            os.chdir(here)
    for c, (n, spg, world, rank, epoch, seed) in enumerate(GROUP_CASES):
        s = gs.DistributedGroupSampler(_Flagged(n), samples_per_gpu=spg, num_replicas=world, rank=rank, seed=seed)
        s.set_epoch(epoch)
        arrays[f"group{c}"] = np.array(list(s), dtype=np.int64)
        assert len(arrays[f"group{c}"]) == len(s)
    for c, (n, world, rank) in enumerate(SEQ_CASES):
        s = ds.DistributedSampler(_Flagged(n), num_replicas=world, rank=rank, shuffle=False)
        arrays[f"seq{c}"] = np.array(list(s), dtype=np.int64)
    return arrays


def main():
    if not ref_stubs.reference_available():
        raise SystemExit("needs the reference checkout (build container only)")
    arrays = generate()
    path = os.path.join(HERE, NAME)
    if "--check" in sys.argv[1:]:
        ref = np.load(path)
        bad = [k for k in ref.files if k not in arrays] + [k for k in arrays if k not in ref.files]
        for k, v in arrays.items():
            v = np.asarray(v)
            if k in ref.files and not (ref[k].shape == v.shape and ref[k].dtype == v.dtype and ref[k].tobytes() == v.tobytes()):
                bad.append(k)
        print("F22 regeneration:", "bit-identical" if not bad else f"MISMATCH in {bad}", f"({len(arrays)} arrays)")
        raise SystemExit(1 if bad else 0)
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
