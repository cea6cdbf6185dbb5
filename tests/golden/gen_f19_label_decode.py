"""Golden F19: the reference's label loaders on one seeded sample of raw label bytes, run from the reference's own module.

    python tests/golden/gen_f19_label_decode.py            writes tests/golden/f19_label_decode.npz
    python tests/golden/gen_f19_label_decode.py --check    regenerates and compares with the committed file bit for bit

Build container only (needs the reference checkout that ref_stubs.py names).  Recipe of gen_f18_train_pipeline.py:
datasets/pipelines/loading.py is imported from where it lies; its third-party imports are the stand-ins of ref_stubs.py.  What
runs is LoadDepth.__call__ (loading.py:84-93) and LoadSeg.__call__ (:132-162, with red_green_yellow :96-113) for
seg_label_idxs = [1, 4, 5, 6, 7, 8, 10, 12, 18] (configs/thinktwice.py:108), with `load_img` replaced ON THE INSTANCES by the
arrays of synth.raw_label_bytes(19, 4, 96, 160) -- PNG file decoding is not what is pinned -- and results['img'] its RGB frames.

cv2 is not installed: cv2.cvtColor / cv2.inRange / cv2.COLOR_RGB2HSV are the stand-ins of tests/labels_ref.py, so the HSV
conversion is NOT pinned by this file ([3P], README_f19.md).  np.bool8, which numpy 2 removed and loading.py:104,108 uses, is
aliased to np.bool_ in this process only.  The file holds data only: the depth maps f32 and the class maps as uint8.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_stubs  # noqa: E402

NAME = "f19_label_decode.npz"
SEED, N, H, W = 19, 4, 96, 160
SEG_LABEL_IDXS = [1, 4, 5, 6, 7, 8, 10, 12, 18]
CAMERAS = ["rgb_front", "rgb_left", "rgb_right", "rgb_back"]


def generate():
    import labels_ref
    from thinktwice_amd import synth
    if not hasattr(np, "bool8"):
        np.bool8 = np.bool_
    ref_stubs.install()
    cv2 = sys.modules["cv2"]
    cv2.cvtColor, cv2.inRange, cv2.COLOR_RGB2HSV = labels_ref.rgb2hsv_u8, labels_ref.in_range, labels_ref.COLOR_RGB2HSV
    for name in ("matplotlib", "matplotlib.pyplot", "mmcv.parallel", "mmdet.datasets", "mmdet.datasets.builder",
                 "mmdet3d.datasets", "mmdet3d.datasets.pipelines", "mmdet3d.datasets.pipelines.loading", "PIL", "PIL.Image"):
        if name not in sys.modules:
            ref_stubs._mod(name)
    sys.modules["mmdet.datasets.builder"].PIPELINES = ref_stubs._Registry("pipelines")
    sys.modules["mmcv.parallel"].DataContainer = lambda x, **k: x
    sys.modules["mmdet3d.datasets.pipelines.loading"].LoadPointsFromFile = object          # (a base class of LoadPoints, unused)
    path = os.path.join(ref_stubs.OLT, "code", "datasets", "pipelines", "loading.py")
    spec = importlib.util.spec_from_file_location("ttref_loading", path)
    ld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ld)

    depth_rgb, tags, rgb = synth.raw_label_bytes(SEED, N, H, W)

    def by_camera(arrays):
        def load_img(filename):                              # <scene>/<camera>/<frame>.png
            kind = os.path.basename(os.path.dirname(filename))
            return arrays[[c.split("_", 1)[1] for c in CAMERAS].index(kind.split("_", 1)[1])]
        return load_img

    results = {"scene_token": "scene", "frame_idx": SEED, "img": [rgb[n] for n in range(N)]}
    load_depth = ld.LoadDepth(is_local=True, camera_names=CAMERAS)
    load_depth.load_img = by_camera(depth_rgb)
    load_seg = ld.LoadSeg(is_local=True, camera_names=CAMERAS, seg_label_idxs=SEG_LABEL_IDXS)
    load_seg.load_img = by_camera(tags)
    results = load_seg(load_depth(results))
    depth, seg = np.stack(results["depth"]), np.stack(results["seg"])
    assert depth.shape == seg.shape == (N, H, W) and depth.dtype == seg.dtype == np.float32
    assert np.array_equal(seg, seg.astype(np.uint8)) and seg.max() <= 10
    # the sample must exercise what the fixture is for: every light type, a component under 20 pixels, the tag 1 -> 0 quirk
    assert all((seg == c).any() for c in (8, 9, 10)) and (seg[tags == 18] == 0).any()
    assert (tags == 1).any() and (seg[tags == 1] == 0).all()
    return dict(seed=np.array([SEED]), shape=np.array([N, H, W]), seg_label_idxs=np.array(SEG_LABEL_IDXS), depth=depth,
                seg=seg.astype(np.uint8))


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
        print("F19 regeneration:", "bit-identical" if not bad else f"MISMATCH in {bad}", f"({len(arrays)} arrays)")
        raise SystemExit(1 if bad else 0)
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
