"""A dataset tree on disk for the loader tests (test_dataset_cpu.py, test_loader.py): three routes of 8, 9 and 10 frames in
three towns, laid out as CarlaDataset expects it --

    <tmp>/dataset/dataset_metadata.pkl
    <tmp>/dataset/<town>/<route>/measurements/NNNN.json  supervision/NNNN.npy  lidar/NNNN.npy
    <tmp>/dataset/<town>/<route>/rgb_front/NNNN.png ... depth_front/NNNN.png ... seg_front/NNNN.png ...
    <tmp>/work/                     the reference's working directory: DatasetIndex(root=) and the "../dataset/..." paths

Frames are 900 x 1600 (the undistortion map fixes that size).  Every file's pixels encode where it belongs, so that a swapped
or misordered file shows in the output: a camera frame is one flat colour `rgb_colour(route, frame, camera)` with a brighter
block in its middle; a depth file is the flat 24-bit code `depth_code(...)`; a seg file is one tag of the config's list with a
block of the next.  Colours differ by at least 6 grey levels between any two (route, frame, camera).

The files are written with filter type 0 on every row, as png_cases.write_png does by default, and go through
png_cases.png_file; the scanlines are assembled from bands of equal rows (`_png`), because write_png's row loop takes 0.3 s
for a frame of this size and the tree has 324."""
import json
import os
import pickle
import zlib

import numpy as np

import png_cases

H, W = 900, 1600
CAMERAS = ["rgb_front", "rgb_left", "rgb_right", "rgb_back"]
# (town, route key as dataset_metadata.pkl holds it, frames)
ROUTES = [("town01_00", "../town01_00/routes_a", 8), ("town03_00", "../town03_00/routes_c", 9), ("town06_00", "../town06_00/routes_b", 10)]
SEG_LABEL_IDXS = [1, 4, 5, 6, 7, 8, 10, 12, 18]
PRED_LEN = 4
CFG = {"pred_len": PRED_LEN, "history_query_index_lis": [-1, 0], "is_local": True, "is_full": False,
       "max_sample_per_town": {"town01": 1e9, "town03": 1e9, "town06": 1e9}, "camera_names": CAMERAS,
       "seg_label_idxs": SEG_LABEL_IDXS}
FEATURES = 256
GRID_SHAPES = [(1,), (1,), (32, 21, 21), (64, 10, 10), (128, 4, 4), (256, 2, 2)]


def rgb_colour(route, frame, camera):
    return (24 + 12 * frame, 40 + 70 * route, 30 + 60 * camera)


def depth_code(route, frame, camera):
    """(r, g, b) of the depth file: (r + 256 g + 65536 b) / (2^24 - 1) * 1000 metres, 1.5 .. 40 m."""
    return (7 * frame + 3 * camera, 11 * route + 5 * frame, 1 + 2 * camera + (frame & 1))


def seg_tags(route, frame, camera):
    k = route + frame + camera
    return SEG_LABEL_IDXS[k % 8], SEG_LABEL_IDXS[(k + 1) % 8]                    # (never the traffic-light tag)


BAND = 50                   # rows; every image below is bands of BAND equal rows


def _png(channels, bands):
    """A file of `bands` = [(one row's pixel bytes, number of BAND-row bands)], filter type 0 on every row.  The zlib stream
    is written band by band, each closed by a full flush, so that a band's bytes are compressed once and repeated: one valid
    stream (what png_cases.COMPRESSORS["flushes"] exercises), a few milliseconds per 900 x 1600 file instead of 45."""
    stream, adler, rows = [b"\x78\x01"], 1, 0
    for row, count in bands:
        lines = (b"\0" + row) * BAND
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        stream.append((co.compress(lines) + co.flush(zlib.Z_FULL_FLUSH)) * count)
        for _ in range(count):
            adler = zlib.adler32(lines, adler)
        rows += BAND * count
    stream.append(b"\x03\x00" + adler.to_bytes(4, "big"))
    return png_cases.png_file(len(bands[0][0]) // channels, rows, channels, b"".join(stream))


def frame_bands(route, frame, camera):
    """(rgb, depth, seg): the (channels, bands) of one camera's three files of one frame."""
    c = rgb_colour(route, frame, camera)
    plain, lit = bytes(c) * W, bytes(c) * 600 + bytes(v + 5 for v in c) * 400 + bytes(c) * 600
    a, b = seg_tags(route, frame, camera)
    return ((3, [(plain, 7), (lit, 4), (plain, 7)]), (3, [(bytes(depth_code(route, frame, camera)) * W, 18)]),
            (1, [(bytes([a]) * W, 6), (bytes([a]) * 400 + bytes([b]) * 500 + bytes([a]) * 700, 4), (bytes([a]) * W, 8)]))


def frame_images(route, frame, camera):
    """(rgb [H, W, 3], depth [H, W, 3], seg [H, W]) uint8 of one camera of one frame: what the three files decode to."""
    out = []
    for channels, bands in frame_bands(route, frame, camera):
        rows = np.concatenate([np.repeat(np.frombuffer(row, np.uint8)[None], BAND * n, axis=0) for row, n in bands])
        out.append(rows.reshape(H, W, 3) if channels == 3 else rows.reshape(H, W))
    return out


def cloud(route, frame):
    """(n, 4) f32, n = 2000 + 7 frame + 13 route: the intensity column carries route + frame / 100."""
    rng = np.random.default_rng(1000 * route + frame)
    n = 2000 + 7 * frame + 13 * route
    p = np.empty((n, 4), np.float32)
    p[:, 0] = rng.uniform(-8, 30, n)
    p[:, 1] = rng.uniform(-19, 19, n)
    p[:, 2] = rng.uniform(-3, 3, n)
    p[:, 3] = route + frame / 100
    return p


def measurement(route, frame, rng):
    return {"x": 100.0 * route + 1.5 * frame + rng.normal(), "y": -50.0 + 0.7 * frame + rng.normal(),
            "theta": float("nan") if (route, frame) == (1, 2) else 0.3 * route + 0.05 * frame, "speed": float(rng.uniform(0, 8)),
            "x_target": 100.0 * route + 1.5 * frame + 20.0, "y_target": -45.0,
            "target_command": -1 if (route + frame) % 5 == 0 else 1 + (route + frame) % 6,
            "acceleration": rng.normal(size=3).tolist(), "angular_velocity": rng.normal(size=3).tolist()}


def supervision(route, frame, rng):
    f32 = lambda a: np.asarray(a, np.float32)                                   # noqa: E731
    return {"action": f32(rng.uniform(-1, 1, 3)), "action_mu": f32(rng.uniform(0.5, 4, 2)), "action_sigma": f32(rng.uniform(0.5, 4, 2)),
            "only_ap_brake": (route + frame) % 3 == 0, "value": np.float32(rng.normal()), "features": f32(rng.normal(size=FEATURES)),
            "cnn_features": [f32(rng.normal(size=s)) for s in GRID_SHAPES]}


def write_tree(tmp):
    """Write the tree under `tmp` -> dict(root=<tmp>/work, metadata=<path of dataset_metadata.pkl>, dataset=<tmp>/dataset)."""
    tmp = str(tmp)
    data_dir = os.path.join(tmp, "dataset")
    os.makedirs(os.path.join(tmp, "work"))
    metadata = {}
    for r, (town, route, L) in enumerate(ROUTES):
        metadata.setdefault(town, {})[route] = L
        d = os.path.join(data_dir, route[3:])
        kinds = ["measurements", "supervision", "lidar"] + [c.replace("rgb", k) for k in ("rgb", "depth", "seg") for c in CAMERAS]
        for k in kinds:
            os.makedirs(os.path.join(d, k))
        rng = np.random.default_rng(77 + r)
        for f in range(L):
            name = f"{f:04d}"
            with open(os.path.join(d, "measurements", name + ".json"), "w") as fh:
                json.dump(measurement(r, f, rng), fh)
            np.save(os.path.join(d, "supervision", name + ".npy"), np.array(supervision(r, f, rng), dtype=object), allow_pickle=True)
            np.save(os.path.join(d, "lidar", name + ".npy"), cloud(r, f))
            for c, cam in enumerate(CAMERAS):
                for kind, (channels, bands) in zip(("rgb", "depth", "seg"), frame_bands(r, f, c)):
                    with open(os.path.join(d, cam.replace("rgb", kind), name + ".png"), "wb") as fh:
                        fh.write(_png(channels, bands))
    path = os.path.join(data_dir, "dataset_metadata.pkl")
    with open(path, "wb") as fh:
        pickle.dump(metadata, fh)
    return {"root": os.path.join(tmp, "work"), "metadata": path, "dataset": data_dir}


def route_number(route_path):
    """The index into ROUTES of a data_infos route string."""
    return [r for r, (_, route, _) in enumerate(ROUTES) if route_path.endswith(route[3:])][0]


def png_files(dataset_dir):
    """Every PNG file of the tree, sorted."""
    out = []
    for base, _, names in os.walk(dataset_dir):
        out += [os.path.join(base, n) for n in names if n.endswith(".png")]
    return sorted(out)
