"""Golden F21: three PNG files as PIL writes them and the arrays the reference's loaders return for them.

    python tests/golden/gen_f21_png_decode.py            writes tests/golden/f21_png_decode.npz
    python tests/golden/gen_f21_png_decode.py --check    runs the reference's loaders over the COMMITTED file bytes and compares
                                                         with the committed arrays bit for bit

Build container only (needs the reference checkout that ref_stubs.py names, and PIL).  Recipe of gen_f19_label_decode.py:
datasets/pipelines/loading.py is imported from where it lies; its third-party imports are the stand-ins of ref_stubs.py, but
PIL is the real one.  The files are written the way the dataset's collector writes them, `Image.fromarray(a).save(path)`
(roach_ap_agent_data_collection.py:574-585), into a temporary <scene>/<camera>/<frame>.png tree; what runs is
LoadMultiImages(is_local=True).load_img (loading.py:40-44) for the camera frame and the depth-coded image and
LoadSeg(is_local=True).load_img (:127-131) for the tag map.  45 x 80 pixels: the three arrays of
synth.raw_label_bytes(21, 1, 45, 80) -- the depth code with every byte random is the file in which PIL's encoder also picks
filter type 0; on the smoother two it picks 1, 2 and 4, and it never picked 3 on any frame tried.

--check does not rewrite the files: their bytes depend on the PIL and zlib versions, the decode of given bytes does not.  The
file holds data only: the file bytes as uint8 arrays, the arrays, each file's per-row filter types, and PIL's version.
"""
import importlib.util
import os
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_stubs  # noqa: E402

NAME = "f21_png_decode.npz"
SEED, H, W = 21, 45, 80
KINDS = {"rgb": "rgb_front", "depth": "depth_front", "seg": "seg_front"}


def source_arrays():
    from thinktwice_amd import synth
    depth, tags, rgb = synth.raw_label_bytes(SEED, 1, H, W)
    return {"rgb": rgb[0], "depth": depth[0], "seg": tags[0]}


def reference_loaders():
    import PIL.Image  # noqa: F401  (the real one, before the stand-ins fill what is missing)
    ref_stubs.install()
    for name in ("matplotlib", "matplotlib.pyplot", "mmcv.parallel", "mmdet.datasets", "mmdet.datasets.builder",
                 "mmdet3d.datasets", "mmdet3d.datasets.pipelines", "mmdet3d.datasets.pipelines.loading"):
        if name not in sys.modules:
            ref_stubs._mod(name)
    sys.modules["mmdet.datasets.builder"].PIPELINES = ref_stubs._Registry("pipelines")
    sys.modules["mmcv.parallel"].DataContainer = lambda x, **k: x
    sys.modules["mmdet3d.datasets.pipelines.loading"].LoadPointsFromFile = object
    path = os.path.join(ref_stubs.OLT, "code", "datasets", "pipelines", "loading.py")
    spec = importlib.util.spec_from_file_location("ttref_loading", path)
    ld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ld)
    images = ld.LoadMultiImages(is_local=True)
    return {"rgb": images.load_img, "depth": images.load_img, "seg": ld.LoadSeg(is_local=True).load_img}


def load_through_reference(files):
    """{kind: file bytes} -> {kind: the array the reference's loader returns}."""
    loaders = reference_loaders()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for kind, data in files.items():
            path = os.path.join(tmp, "scene", KINDS[kind], str(SEED).zfill(4) + ".png")
            os.makedirs(os.path.dirname(path))
            with open(path, "wb") as f:
                f.write(data)
            out[kind] = loaders[kind](path)
    return out


def filter_types(data):
    import png_ref
    w, h, c, stream = png_ref.parse(data)
    return np.frombuffer(zlib.decompress(stream), dtype=np.uint8).reshape(h, 1 + w * c)[:, 0].copy()


def generate():
    import io

    import PIL
    from PIL import Image
    src = source_arrays()
    files = {}
    for kind, a in src.items():
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="PNG")
        files[kind] = buf.getvalue()
    loaded = load_through_reference(files)
    arrays = {"shape": np.array([H, W]), "seed": np.array([SEED]), "pil_version": np.array(PIL.__version__)}
    used = set()
    for kind in KINDS:
        assert loaded[kind].dtype == np.uint8 and np.array_equal(loaded[kind], src[kind]), kind
        arrays[f"{kind}_file"] = np.frombuffer(files[kind], dtype=np.uint8)
        arrays[f"{kind}_array"] = loaded[kind]
        arrays[f"{kind}_filters"] = filter_types(files[kind])
        used |= set(arrays[f"{kind}_filters"].tolist())
    # the fixture must hold every filter type PIL's encoder chose on full-size dataset-like frames (0, 1, 2 and 4 were seen)
    assert used >= {0, 1, 2, 4}, f"filter types {sorted(used)}: enlarge the images"
    return arrays


def main():
    if not ref_stubs.reference_available():
        raise SystemExit("needs the reference checkout (build container only)")
    path = os.path.join(HERE, NAME)
    if "--check" in sys.argv[1:]:
        ref = np.load(path)
        loaded = load_through_reference({k: ref[f"{k}_file"].tobytes() for k in KINDS})
        src = source_arrays()
        bad = [k for k in KINDS if not (loaded[k].shape == ref[f"{k}_array"].shape and loaded[k].dtype == ref[f"{k}_array"].dtype
                                        and np.array_equal(loaded[k], ref[f"{k}_array"]) and np.array_equal(loaded[k], src[k])
                                        and np.array_equal(filter_types(ref[f"{k}_file"].tobytes()), ref[f"{k}_filters"]))]
        print("F21 check:", "bit-identical" if not bad else f"MISMATCH in {bad}", f"({len(KINDS)} files)")
        raise SystemExit(1 if bad else 0)
    arrays = generate()
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB); filter types per file:",
          {k: sorted(set(arrays[f'{k}_filters'].tolist())) for k in KINDS})


if __name__ == "__main__":
    main()
