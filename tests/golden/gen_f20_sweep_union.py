"""Golden F20: the reference's own `union2one` (open_loop_training/code/datasets/carla_dataset.py:263-334, with get_ego_shift
:252-259) on a few tiny seeded queues, run from the reference's own module.

    python tests/golden/gen_f20_sweep_union.py            writes tests/golden/f20_sweep_union.npz
    python tests/golden/gen_f20_sweep_union.py --check    regenerates and compares with the committed file bit for bit

Build container only (needs the reference checkout that ref_stubs.py names).  Recipe of gen_f19_label_decode.py:
datasets/carla_dataset.py is imported from where it lies, under a synthetic parent package so that datasets/__init__.py does
not run; its third-party imports are the stand-ins of ref_stubs.py plus the few set below.  What is NOT the reference's:
  * mmcv.parallel.DataContainer is a holder with a `.data` attribute (all union2one uses of it);
  * the full-queue pipeline (IDAImageTransform + ImageTransformMulti in the reference's config) is a stand-in that only sets
    every frame's `lidar2cam`, f32 [N, 4, 4] as transform.py:245 holds it, here thinktwice_amd.calib.camera_tables()'s;
  * `img` is a one-element tensor per frame: the images are not what is pinned.
The queues: T = 2 and T = 3; clouds of 0, 1, 5 and 67 points, an empty key sweep among them; intensities up to 3, so that the
intensity-as-w quirk of :323 shows; yaw differences on both sides of +-pi.  The file holds data only: per queue the input
can_bus vectors and clouds, and the reference's points, curr2key, currlidar2keycam, can_bus and prev_bev."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_stubs  # noqa: E402

NAME = "f20_sweep_union.npz"
SEED = 20
# (points per sweep oldest first, yaw per frame in radians)
QUEUES = [([5, 67], [-3.0, 3.0]),                   # key - curr = 6.0: past +pi
          ([0, 1], [0.25, 0.125]),
          ([67, 0, 5], [3.1, -3.1, 0.5]),           # -3.6 and +2.6 against the key frame; an empty middle sweep
          ([1, 5, 0], [-2.0, 2.5, -2.75])]          # an empty key sweep; -0.75 and -5.25: past -pi


class _Held:
    def __init__(self, data, **kw):
        self.data = data


def _load_reference():
    ref_stubs.install()
    for name in ("matplotlib", "matplotlib.pyplot", "mmcv.parallel", "mmdet.datasets", "mmdet3d.datasets",
                 "mmdet3d.datasets.pipelines", "PIL", "PIL.Image", "nuscenes", "nuscenes.eval", "nuscenes.eval.common",
                 "nuscenes.eval.common.utils"):
        if name not in sys.modules:
            ref_stubs._mod(name)
    sys.modules["mmcv.parallel"].DataContainer = _Held
    sys.modules["mmdet.datasets"].DATASETS = ref_stubs._Registry("datasets")
    sys.modules["mmdet.datasets"].CustomDataset = object
    pkg = types.ModuleType(f"{ref_stubs.REF_PKG}.datasets")          # (datasets/__init__.py imports the samplers and builders)
    pkg.__path__ = [os.path.join(ref_stubs.OLT, "code", "datasets")]
    sys.modules[pkg.__name__] = pkg
    path = os.path.join(ref_stubs.OLT, "code", "datasets", "carla_dataset.py")
    spec = importlib.util.spec_from_file_location(f"{pkg.__name__}.carla_dataset", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def make_queues():
    """The inputs, seeded: [(can_bus [T, 18] float64, [cloud (n, 4) f32 per frame])]."""
    rng = np.random.default_rng(SEED)
    out = []
    for counts, yaws in QUEUES:
        T = len(counts)
        can_bus = rng.normal(size=(T, 18))
        can_bus[:, :2] = rng.uniform(-200, 200, 2) + np.cumsum(rng.uniform(-3, 3, (T, 2)), axis=0)
        can_bus[:, -2] = yaws
        can_bus[:, -1] = can_bus[:, -2] / np.pi * 180                # carla_dataset.py:145-146
        clouds = []
        for n in counts:
            p = np.empty((n, 4), np.float32)
            p[:, :3] = rng.uniform(-40, 40, (n, 3))
            p[:, 3] = rng.uniform(0, 3, n)
            clouds.append(p)
        out.append((can_bus, clouds))
    return out


def generate():
    import torch
    from thinktwice_amd import calib
    cd = _load_reference()
    lidar2cam = torch.from_numpy(np.ascontiguousarray(calib.camera_tables()[1], dtype=np.float32))

    def full_queue_pipeline(queue):
        for frame in queue:
            frame["img_metas"].data["lidar2cam"] = lidar2cam
        return queue

    arrays = dict(seed=np.array([SEED]), lidar2cam=lidar2cam.numpy().copy())
    for q, (can_bus, clouds) in enumerate(make_queues()):
        T = len(clouds)
        queue = [{"img": torch.zeros(1), "points": torch.from_numpy(clouds[t].copy()),
                  "img_metas": _Held({"can_bus": can_bus[t].copy()})} for t in range(T)]
        res = cd.union2one(full_queue_pipeline, queue)
        metas = res["img_metas"].data
        points = res["points"].data.numpy()
        assert points.dtype == np.float32 and points.shape == (1, sum(len(c) for c in clouds), 5)
        assert all(m["points_size"] == [len(c) for c in clouds] for m in metas)
        arrays[f"q{q}_can_bus_in"] = can_bus
        arrays[f"q{q}_sizes"] = np.array([len(c) for c in clouds])
        arrays[f"q{q}_clouds_in"] = np.concatenate(clouds)
        arrays[f"q{q}_points"] = points
        arrays[f"q{q}_curr2key"] = np.stack([m["curr2key"].numpy() for m in metas])
        arrays[f"q{q}_currlidar2keycam"] = np.stack([m["currlidar2keycam"].numpy() for m in metas])
        arrays[f"q{q}_can_bus"] = np.stack([np.asarray(m["can_bus"], np.float64) for m in metas])
        arrays[f"q{q}_prev_bev"] = np.array([bool(m["prev_bev"]) for m in metas])
        assert arrays[f"q{q}_curr2key"].dtype == arrays[f"q{q}_currlidar2keycam"].dtype == np.float32
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
            if k in ref.files and not (ref[k].shape == np.asarray(v).shape and ref[k].dtype == np.asarray(v).dtype
                                       and np.array_equal(ref[k].view(np.uint8), np.ascontiguousarray(v).view(np.uint8))):
                bad.append(k)
        print("F20 regeneration:", "bit-identical" if not bad else f"MISMATCH in {bad}", f"({len(arrays)} arrays)")
        raise SystemExit(1 if bad else 0)
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
