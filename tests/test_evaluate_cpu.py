"""evaluate.summarize / merge_raw / the command line and the runner's save_best rule: host code only."""
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eval_ref as E  # noqa: E402


def _raw(C=4, S=2, n=3):
    conf = [[5, 1, 0, 0], [2, 7, 0, 0], [0, 0, 0, 0], [0, 3, 0, 0]][:C]
    return OrderedDict(seg_conf=conf, seg_bad_label=2, seg_nonfinite=1, depth=[10, 4, 7, 13, 1], num_samples=n, dec_nonfinite=1,
                       dec_sums=[float(i) + 0.125 for i in range(8 * S + 1)], d_step=0.5)


def test_summarize_is_the_restated_arithmetic_and_zero_union_classes_stay_out():
    from thinktwice_amd import evaluate
    names = ["a", "b", "c", "d"]
    raw = _raw()
    got = evaluate.summarize(raw, names)
    want = E.summarize(raw, names, 0.5)
    assert list(got) == list(want)
    for k in want:
        assert got[k] == want[k], k
    assert got["seg_iou"]["c"] is None                                # no label and no prediction of class c
    assert got["seg_iou"]["d"] == 0.0                                 # labelled, never predicted: a union, no intersection
    assert got["seg_iou"]["a"] == 5 / 8 and got["seg_iou"]["b"] == 7 / 13
    assert got["seg_miou"] == (5 / 8 + 7 / 13 + 0.0) / 3
    assert got["seg_pixel_acc"] == 12 / 18
    assert got["depth_top1"] == 0.4 and got["depth_within1"] == 0.7 and got["depth_mae_m"] == 13 * 0.5 / 10
    assert got["wp_ade_0"] == 0.125 / 3 and got["wp_fde_1"] == 9.125 / 3 and got["speed_mae"] == 16.125 / 3
    assert got["num_samples"] == 3 and got["nonfinite"] == 1 and got["seg_bad_label"] == 2
    flat = evaluate.scalar_metrics(got)
    assert "seg_iou_c" not in flat and flat["seg_iou_d"] == 0.0 and "num_samples" not in flat and flat["seg_miou"] == got["seg_miou"]


def test_summarize_of_nothing_is_nan_not_a_division_error():
    from thinktwice_amd import evaluate
    raw = _raw()
    raw["depth"] = [0, 0, 0, 0, 0]
    raw["num_samples"] = 0
    raw["seg_conf"] = [[0] * 4 for _ in range(4)]
    got = evaluate.summarize(raw, ["a", "b", "c", "d"])
    for k in ("depth_top1", "depth_within1", "depth_mae_m", "wp_ade_0", "speed_mae", "seg_miou", "seg_pixel_acc"):
        assert math.isnan(got[k]), k
    assert all(v is None for v in got["seg_iou"].values())


def test_merge_raw_adds_integers_exactly_and_sums_in_rank_order():
    from thinktwice_amd import evaluate
    a, b, c = _raw(), _raw(), _raw()
    b["seg_conf"][0][0] = 2 ** 40
    a["dec_sums"][0], b["dec_sums"][0], c["dec_sums"][0] = 1e16, 1.0, -1e16
    m = evaluate.merge_raw([a, b, c])
    assert m["seg_conf"][0][0] == 2 ** 40 + 10 and m["depth"] == [30, 12, 21, 39, 3] and m["num_samples"] == 9
    assert m["dec_sums"][0] == (1e16 + 1.0) - 1e16 and m["dec_sums"][1] == 1.125 * 3
    assert evaluate.merge_raw([a]) == a


def test_class_names_follow_the_label_decoder():
    from thinktwice_amd import data_config, evaluate, labels
    names = evaluate.seg_class_names()
    idxs = data_config.DATA["seg_label_idxs"]
    assert len(names) == 12 and len(set(names)) == 12
    conf = labels.seg_decode_conf(idxs)
    assert names[conf.light_base] == "traffic_light" and names[conf.light_base + 1] == "traffic_light_red"
    assert names[conf.light_base + 2] == "traffic_light_green" and names[conf.class_of_tag[7]] == "road"
    assert names[0].startswith("background")


def test_command_line_parsing():
    from thinktwice_amd import evaluate, train
    a = evaluate.parse_args(["--data-root", "r", "--load-from", "c.pth"])
    assert (a.dtype, a.against, a.towns, a.batch_size, a.out, a.metadata) == ("f32x3h", None, None, 8, None, None)
    a = evaluate.parse_args(["--data-root", "r", "--dtype", "f32x3", "--against", "f32", "--towns", "town02_val", "town05_val",
                             "--batch-size", "2", "--out", "m.json", "--final-dim", "128", "256"])
    assert (a.dtype, a.against, a.towns, a.batch_size, a.out, a.final_dim) == ("f32x3", "f32", ["town02_val", "town05_val"], 2,
                                                                              "m.json", [128, 256])
    for bad in (["--load-from", "c.pth"], ["--data-root", "r", "--dtype", "f64"], ["--data-root", "r", "--batch-size", "0"],
                ["--data-root", "r", "--dtype", "f32", "--against", "f32"]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(bad)
    t = train.assemble(train.parse_args(["--data-root", "r", "--work-dir", "w", "--metrics", "--save-best", "seg_miou:greater"]))
    assert t["runner"]["metrics"] is True and t["runner"]["save_best"] == "seg_miou" and t["runner"]["save_best_rule"] == "greater"
    t = train.assemble(train.parse_args(["--data-root", "r", "--work-dir", "w", "--save-best", "wp_ade_5"]))
    assert t["runner"]["save_best"] == "wp_ade_5" and t["runner"]["save_best_rule"] == "less" and "metrics" not in t["runner"]
    with pytest.raises(SystemExit):
        train.parse_args(["--data-root", "r", "--work-dir", "w", "--save-best", "x:upwards"])


def test_the_save_best_rule():
    from thinktwice_amd import runner
    assert runner.is_better(1.0, None) and runner.is_better(1.0, None, "greater")
    assert runner.is_better(0.5, 1.0) and not runner.is_better(1.5, 1.0) and not runner.is_better(1.0, 1.0)
    assert runner.is_better(1.5, 1.0, "greater") and not runner.is_better(0.5, 1.0, "greater") and not runner.is_better(1.0, 1.0, "greater")
    assert not runner.is_better(float("nan"), 1.0) and not runner.is_better(float("nan"), 1.0, "greater")
    with pytest.raises(ValueError):
        runner.is_better(1.0, 2.0, "upwards")
    assert runner.parse_save_best("loss") == ("loss", "less") and runner.parse_save_best("seg_miou:greater") == ("seg_miou", "greater")
    # on a hand-made pair of validation values the two rules keep different epochs
    vals = [0.3, 0.7]
    for rule, want in (("less", 0), ("greater", 1)):
        best, kept = None, None
        for e, v in enumerate(vals):
            if runner.is_better(v, best, rule):
                best, kept = v, e
        assert kept == want
    with pytest.raises(ValueError, match="save_best_rule"):
        runner.EpochRunner(None, [], work_dir=".", save_best_rule="upwards")


def test_the_restated_kernels_on_hand_made_cases():
    conf, bad, nf = E.seg_confusion(np.array([[[[0, 2, 2, 9], [1, 0, 0, 9], [np.nan, 0, 0, 9], [0, 0, 1, 9]]]], np.float32),
                                    np.array([[[1, 255, 0, 3]]], np.float32), 3, 1)
    assert conf.tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]] and bad == 1 and nf == 1
    sums, counts = E.decoder(np.zeros((2, 1, 4, 2)), np.zeros((2, 1, 2)), np.ones((2, 1, 2)), [[0.5], [np.nan]],
                             np.full((2, 4, 2), [3.0, 4.0]), np.ones((2, 2)), np.ones((2, 2)), [5.0, 1.0])
    assert counts == [1, 1] and sums.tolist() == [5.0, 5.0, 3.0, 4.0, 1.0, 1.0, 0.0, 0.0, 1.0]
    assert E.pair_deviation([1.0, -3.0, np.inf], [1.5, -3.0, 0.0]) == (np.float32(0.5), np.float32(3.0), 1)
