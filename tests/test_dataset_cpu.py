"""CPU: the host side of the sample assembly (thinktwice_amd/dataset.py, the reader job and the evaluation parameters of
thinktwice_amd/loader.py) against golden F22 -- what the reference's own CarlaDataset, DistributedGroupSampler and
DistributedSampler returned (tests/golden/gen_f22_dataset.py) -- in every bit, and the collate, the cloud reader and the
read counts against what they are specified to be."""
import collections
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import gen_f22_dataset as G  # noqa: E402  (its input helpers; nothing of the reference is imported)
from thinktwice_amd import calib, dataset, synth  # noqa: E402


@pytest.fixture(scope="module")
def f22():
    return np.load(os.path.join(HERE, "golden", G.NAME))


@pytest.fixture(scope="module")
def routes(f22, tmp_path_factory):
    """The golden's routes written out again from its input arrays -> [route directory]."""
    return G.write_routes(str(tmp_path_factory.mktemp("f22")), f22)


def _same_bits(got, want, what):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), what


def test_frame_info_equals_the_reference_in_every_bit_golden_f22(f22, routes):
    assert int(f22["seed"][0]) == G.SEED and len(f22["info_cases"]) == 5
    seen = collections.Counter()
    for c, (r, frame, current) in enumerate(f22["info_cases"].tolist()):
        name = "../dataset/" + str(f22["routes"][r])[3:]
        res = dataset.frame_info(routes[r], frame, bool(current), int(f22["pred_len"][0]), name=name)
        got = G.flatten_info(res, f"info{c}_")
        want = sorted(k for k in f22.files if k.startswith(f"info{c}_"))
        assert sorted(got) == want                                               # the same keys
        for k in want:
            _same_bits(got[k], f22[k], k)
        assert got[f"info{c}_can_bus"].dtype == np.float64 and got[f"info{c}_target_command"].dtype == np.int64
        meas = f22[f"r{r}_meas"][frame]
        seen["nan"] += bool(np.isnan(meas[2]))
        seen["void"] += meas[6] == -1
        if np.isnan(meas[2]):
            assert res["input_theta"] == -np.pi / 2
        if meas[6] == -1:
            assert int(res["target_command_raw"]) == 3 and res["target_command"].tolist() == [0, 0, 0, 1, 0, 0]
        if current:
            brake = f22[f"r{r}_only_ap_brake"]
            seen["brake_now"] += bool(brake[frame])
            seen["brake_later"] += int(brake[frame + 1:frame + 5].sum())
            for hit, mu, sg in [(brake[frame], res["action_mu"], res["action_sigma"])] + [
                    (brake[frame + 1 + p], res["future_action_mu"][p], res["future_action_sigma"][p]) for p in range(4)]:
                assert (mu[0] == np.float32(0.8) and sg[0] == np.float32(5.5)) == bool(hit)
    assert min(seen["nan"], seen["void"], seen["brake_now"], seen["brake_later"]) >= 1, seen     # the quirks did occur


def test_dataset_index_equals_the_reference_golden_f22(f22, tmp_path):
    import pickle
    metadata, caps = json.loads(str(f22["index_metadata"])), json.loads(str(f22["index_caps"]))
    towns = [str(t) for t in f22["index_towns"]]
    cases = json.loads(str(f22["index_cases"]))
    assert len(cases) == 4
    for c, case in enumerate(cases):
        cfg = {"pred_len": int(f22["pred_len"][0]), "history_query_index_lis": case["history"], "is_local": True,
               "max_sample_per_town": caps}
        if case["is_full"] is not None:
            cfg["is_full"] = case["is_full"]
        index = dataset.DatasetIndex(metadata, towns, cfg, root="/data/work")
        want = list(zip((str(r) for r in f22[f"index{c}_routes"]), f22[f"index{c}_frames"].tolist()))
        assert index.data_infos == want and len(index) == len(want) and index[0] == want[0] and index[len(want) - 1] == want[-1]
        assert all(isinstance(f, int) for _, f in index.data_infos)
    # the quirks, on case 0: starts at frame 1, town01 overshoots its cap of 5 by one route, r1 (5 frames) and r3, r4 are out
    index = dataset.DatasetIndex(metadata, towns, dict(cfg, history_query_index_lis=[-1, 0], is_full=False))
    per_route = collections.Counter(r for r, _ in index.data_infos)
    assert per_route["../dataset/town01_00/routes_r0"] == 4 and per_route["../dataset/town01_00/routes_r2"] == 5
    assert not any("routes_r1" in r or "routes_r3" in r or "routes_r4" in r for r in per_route)
    assert min(f for _, f in index.data_infos) == 1
    assert index.path("../dataset/town01_00/routes_r0", "lidar") == "../dataset/town01_00/routes_r0/lidar"
    path = tmp_path / "dataset_metadata.pkl"
    path.write_bytes(pickle.dumps(metadata))
    from_file = dataset.DatasetIndex(str(path), towns, dict(cfg, history_query_index_lis=[-1, 0], is_full=False), root="/w")
    assert from_file.data_infos == index.data_infos
    assert from_file.path("../dataset/t/r", "lidar", "0001.npy") == "/w/../dataset/t/r/lidar/0001.npy"
    assert dataset.DatasetIndex(metadata, towns, dict(cfg, is_local=False)).data_infos[0][0] == "../town01_00/routes_r0"


def test_samplers_equal_the_reference_golden_f22(f22):
    for c, (n, spg, world, rank, epoch, seed) in enumerate(f22["group_cases"].tolist()):
        s = dataset.GroupSampler(n, spg, world, rank, None if seed == -1 else seed)
        s.set_epoch(epoch)
        got = list(s)
        assert got == f22[f"group{c}"].tolist() and len(s) == len(got), (c, got)
        assert all(isinstance(i, int) for i in got)
    for c, (n, world, rank) in enumerate(f22["seq_cases"].tolist()):
        s = dataset.SequentialSampler(n, world, rank)
        assert list(s) == f22[f"seq{c}"].tolist() and len(s) == len(f22[f"seq{c}"]), c
    assert len(f22["group_cases"]) == 7 and len(f22["seq_cases"]) == 6
    a = dataset.GroupSampler(17, 2, 1, 0, 0)
    first = list(a)
    a.set_epoch(1)
    assert list(a) != first and sorted(set(list(a))) == list(range(17))


# ------------------------------------------------------------------------------------------------------------- collate
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    import dataset_cases as D
    return D.write_tree(tmp_path_factory.mktemp("tree"))


def _index(tree, towns=("town01_00", "town03_00", "town06_00")):
    import dataset_cases as D
    return dataset.DatasetIndex(tree["metadata"], list(towns), D.CFG, root=tree["root"])


def test_collate_targets_is_float32_of_frame_info_in_the_synth_shapes(tree):
    import dataset_cases as D
    index = _index(tree)
    assert len(index) == 3 + 4 + 5 and index[0][1] == 1 and index[3] == ("../dataset/town03_00/routes_c", 1)
    picks = [index[2], index[3], index[11]]                                      # a route's last sample, the next one's first
    infos = [dataset.frame_info(index.path(r), f, True, D.PRED_LEN, name=r) for r, f in picks]
    again = [dataset.frame_info(index.path(r), f, True, D.PRED_LEN, name=r) for r, f in picks]
    got = dataset.collate_targets(infos)
    B = len(picks)
    want = synth.make_train_targets(B)
    want.update({k: v for k, v in synth.make_batch(B, num_points=8, with_img=False).items()
                 if k in ("speed", "target_point", "target_command", "target_command_raw")})

    def shapes(v):
        return [shapes(x) for x in v] if isinstance(v, list) else (tuple(v.shape), v.dtype)

    for k, v in want.items():
        if k in ("depth", "seg"):
            continue                                                             # (built by the device stages)
        assert shapes(got[k]) == shapes(v), k
    assert sorted(got) == sorted(["waypoints", "target_point", "target_command", "target_command_raw", "speed", "future_speed",
                                  "value", "future_value", "feature", "future_feature", "grid_feature", "future_grid_feature",
                                  "action_sigma", "action_mu", "future_action_mu", "future_action_sigma"])   # thinktwice.py:212-218

    def f32(values):
        return np.stack([np.float32(np.asarray(v, dtype=np.float64)) for v in values])

    for k in ("waypoints", "target_point", "speed", "value", "feature", "action_mu", "action_sigma"):
        a = got[k].numpy()
        assert a.dtype == np.float32 and np.array_equal(a, f32([i[k] for i in again]).reshape(a.shape)), k
    assert np.array_equal(got["target_command"].numpy(), f32([i["target_command"].numpy() for i in again]))
    assert got["target_command_raw"].tolist() == [int(i["target_command_raw"]) for i in again]
    for p in range(D.PRED_LEN):
        for k in ("future_action_mu", "future_action_sigma", "future_feature", "future_speed", "future_value"):
            a = got[k][p].numpy()
            assert a.dtype == np.float32 and np.array_equal(a, f32([i[k][p] for i in again]).reshape(a.shape)), (k, p)
        for j in range(6):
            assert np.array_equal(got["future_grid_feature"][p][j].numpy(), f32([i["future_grid_feature"][p][j] for i in again]))
    for j in range(6):
        assert np.array_equal(got["grid_feature"][j].numpy(), f32([i["grid_feature"][j] for i in again]))
    assert got["waypoints"].shape == (B, 4, 2) and got["future_speed"][0].shape == (B,)
    assert infos[0]["waypoints"].dtype == np.float64                             # the rounding happened in the collate


# ----------------------------------------------------------------------------------------------------------- load_cloud
@pytest.mark.parametrize("n", [0, 1, 67])
def test_load_cloud_round_trips_np_save(n):
    a = np.random.default_rng(n).normal(size=(n, 4)).astype(np.float32)
    buf = io.BytesIO()
    np.save(buf, a)
    got = dataset.load_cloud(buf.getvalue(), "x.npy")
    assert got.dtype == np.float32 and got.shape == (n, 4) and np.array_equal(got.view(np.uint32), a.view(np.uint32))
    assert not got.flags.writeable                                               # a view of the file bytes


def test_load_cloud_refuses_other_dtypes_and_shapes():
    for bad in (np.zeros((3, 4), np.float64), np.zeros((3, 5), np.float32), np.zeros(12, np.float32), np.zeros((3, 4), ">f4"),
                np.asfortranarray(np.zeros((3, 4), np.float32))):
        buf = io.BytesIO()
        np.save(buf, bad)
        with pytest.raises(ValueError, match="lidar/0007.npy"):
            dataset.load_cloud(buf.getvalue(), "r/lidar/0007.npy")
    with pytest.raises(ValueError, match="lidar/0007.npy"):
        dataset.load_cloud(b"not a numpy file at all", "r/lidar/0007.npy")
    buf = io.BytesIO()
    np.save(buf, np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="lidar/0007.npy"):
        dataset.load_cloud(buf.getvalue()[:-8], "r/lidar/0007.npy")                # cut short


# ------------------------------------------------------------------------------------------------------------ the loader's host side
def test_eval_branch_ida_parameters_give_the_evaluation_matrix():
    from thinktwice_amd import loader, preprocess
    for fd in ((calib.FINAL_H, calib.FINAL_W), (128, 256), (224, 448)):
        conf = dict(calib.IDA_AUG_CONF, final_dim=fd)
        p = loader.eval_ida_params(conf)
        got = preprocess.ida_mat(p, fd)
        assert got.dtype == np.float32 and np.array_equal(got, calib.eval_ida_mat(fd)) and p.flip is False
        preprocess.check_ida_params([[p]], fd)
    p = loader.eval_ida_params(calib.IDA_AUG_CONF)
    assert (p.resize, p.resized_h, p.resized_w, p.crop_y, p.crop_x) == (0.56, 504, 896, 56, 0)


def test_every_file_is_read_exactly_once_and_only_the_key_frames_labels(tree):
    import dataset_cases as D
    from thinktwice_amd import loader
    index = _index(tree)
    route, frame = index[5]                                                      # routes_c, frame 3
    assert (route, frame) == ("../dataset/town03_00/routes_c", 3)
    reads = collections.Counter()

    def read(path):
        reads[os.path.relpath(path, index.path(route))] += 1
        return dataset.read_file(path)

    T, N, P = 2, 4, 4
    got = loader.read_sample(index.path(route), route, frame, [-1, 0], D.CAMERAS, P, read)
    assert set(reads.values()) == {1}                                            # exactly once each
    kinds = collections.Counter(p.split(os.sep)[0].split("_")[0] for p in reads)
    assert kinds == {"rgb": T * N, "depth": N, "seg": N, "lidar": T, "measurements": 1 + P + (T - 1), "supervision": 1 + P}
    assert sum(reads.values()) == 8 + 4 + 4 + 2 + 6 + 5 == 29
    labels = sorted(p for p in reads if p.startswith(("depth", "seg")))
    assert labels == sorted(f"{c.replace('rgb', k)}/0003.png" for c in D.CAMERAS for k in ("depth", "seg"))   # the key frame's only
    assert sorted(p for p in reads if p.startswith("measurements")) == [f"measurements/{f:04d}.json" for f in (2, 3, 4, 5, 6, 7)]
    assert sorted(p for p in reads if p.startswith("supervision")) == [f"supervision/{f:04d}.npy" for f in (3, 4, 5, 6, 7)]
    assert [os.path.basename(p) for p in got["lidar_paths"]] == ["0002.npy", "0003.npy"]          # oldest frame first
    assert [i["frame_idx"] for i in got["infos"]] == [2, 3] and "waypoints" in got["infos"][1] and "waypoints" not in got["infos"][0]
    assert got["infos"][0]["input_theta"] == -np.pi / 2                          # routes_c frame 2: theta is NaN in the fixture
    assert np.array_equal(got["clouds"][1], D.cloud(1, 3)) and got["rgb"][0][2] == dataset.read_file(got["rgb_paths"][0][2])

    def missing(path):
        if path.endswith(os.path.join("rgb_left", "0002.png")):
            raise FileNotFoundError(2, "No such file or directory", path)
        return dataset.read_file(path)

    with pytest.raises(FileNotFoundError, match="rgb_left/0002.png"):
        loader.read_sample(index.path(route), route, frame, [-1, 0], D.CAMERAS, P, missing)
