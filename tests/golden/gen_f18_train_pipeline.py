"""Golden F18: the reference's TRAINING image pipeline on one seeded sample, run from the reference's own module.

    python tests/golden/gen_f18_train_pipeline.py            writes tests/golden/f18_train_image_pipeline.npz
    python tests/golden/gen_f18_train_pipeline.py --check    regenerates and compares with the committed file bit for bit

Build container only (needs the reference checkout that ref_stubs.py names).  Recipe of gen_golden.py::gen_f17:
datasets/pipelines/transform.py is imported from where it lies; its third-party imports are the stand-ins of ref_stubs.py
(torchvision Resize / Normalize / Compose, the registries) plus cv2.initUndistortRectifyMap -> calib.undistort_rectify_map.
What runs is IDAImageTransform(is_train=True).__call__ (transform.py:275-341: undistortion of frames and of the depth / seg
label maps, one sample_ida_augmentation draw :248-263 per camera, img_transform :346-378 and depth_transform :386-396 with
that draw) followed by ImageTransformMulti(aug=False) (:144,163), with use_depth = use_seg = True, after np.random.seed(18),
on synth.raw_camera_frames(18) and synth.raw_label_maps(18).  The file holds data only: the four draws (logged by wrapping the
instance's sample_ida_augmentation), ida_mats, sampled output values, one full row and column per key-sweep image and per
label map, per-image means.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_stubs  # noqa: E402

NAME = "f18_train_image_pipeline.npz"
SEED = 18
ROW, COL = 200, 431


def generate():
    from thinktwice_amd import calib, synth
    ref_stubs.install()
    cv2 = sys.modules["cv2"]
    cv2.initUndistortRectifyMap = lambda mtx, dist, R, newmtx, size, m1type: calib.undistort_rectify_map(size[0], size[1])
    for name in ("matplotlib", "matplotlib.pyplot", "imgaug", "imgaug.augmenters", "mmcv.parallel", "mmdet.datasets",
                 "mmdet.datasets.builder", "mmdet.datasets.pipelines"):
        ref_stubs._mod(name)
    sys.modules["mmdet.datasets.builder"].PIPELINES = ref_stubs._Registry("pipelines")
    sys.modules["mmcv.parallel"].DataContainer = lambda x, **k: x
    sys.modules["mmdet.datasets.pipelines"].to_tensor = torch.as_tensor
    path = os.path.join(ref_stubs.OLT, "code", "datasets", "pipelines", "transform.py")
    spec = importlib.util.spec_from_file_location("ttref_transform", path)
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)

    cfg = dict(img_size=(448, 896), camera_names=list(calib.CAMERA_NAMES), undistort=True, unreal_coord=True,
               use_depth=True, use_seg=True, num_cams=4, queue_length=2)                        # configs/thinktwice.py:41-120
    raw = synth.raw_camera_frames(seed=SEED)
    depth, seg = synth.raw_label_maps(seed=SEED)
    T_, N = raw.shape[:2]
    queue = [{"img": types.SimpleNamespace(data=raw[t]), "img_metas": types.SimpleNamespace(data={})} for t in range(T_)]
    queue[-1]["depth"] = list(depth)                                                          # np.stack(queue[-1]['depth'])
    queue[-1]["seg"] = list(seg)
    ida = tr.IDAImageTransform(cfg, dict(calib.IDA_AUG_CONF), is_train=True)
    draws, inner = [], ida.sample_ida_augmentation

    def logged():
        resize, resize_dims, crop, flip = inner()
        draws.append([float(resize), resize_dims[1], resize_dims[0], crop[1], crop[0], int(bool(flip))])
        return resize, resize_dims, crop, flip

    ida.sample_ida_augmentation = logged
    np.random.seed(SEED)
    with torch.no_grad():
        queue = ida(queue)
        mats = torch.stack([q["img_metas"].data["ida_mats"] for q in queue]).numpy()            # [T, N, 4, 4]
        queue = tr.ImageTransformMulti(aug=False, batch_size=1)(queue)
    out = torch.stack([q["img"] for q in queue]).numpy()                                        # [T, N, 3, 448, 896]
    d, s = queue[-1]["depth"].numpy(), queue[-1]["seg"].numpy()                                 # [N, 448, 896]
    assert out.shape == (T_, N, 3, 448, 896) and d.shape == s.shape == (N, 448, 896) and len(draws) == N
    rng = np.random.default_rng(1818)
    idx = rng.choice(out.size, size=16384, replace=False).astype(np.int64)
    lidx = rng.choice(d.size, size=8192, replace=False).astype(np.int64)
    arrays = dict(seed=np.array([SEED]),
                  # per camera: resize, resized_h, resized_w, crop_y, crop_x, flip
                  params=np.asarray(draws, dtype=np.float64), ida_mats=mats,
                  sample_idx=idx, sample_val=out.reshape(-1)[idx],
                  per_image_mean=out.mean(axis=(2, 3, 4)), per_image_abs_mean=np.abs(out).mean(axis=(2, 3, 4)),
                  row_200=out[-1, :, :, ROW, :], col_431=out[-1, :, :, :, COL], label_idx=lidx)
    for name, m in (("depth", d), ("seg", s)):
        arrays.update({f"{name}_val": m.reshape(-1)[lidx], f"{name}_row_200": m[:, ROW, :], f"{name}_col_431": m[:, :, COL],
                       f"{name}_mean": m.mean(axis=(1, 2))})
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
                                       and np.array_equal(ref[k], v)):
                bad.append(k)
        print("F18 regeneration:", "bit-identical" if not bad else f"MISMATCH in {bad}", f"({len(arrays)} arrays)")
        raise SystemExit(1 if bad else 0)
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
