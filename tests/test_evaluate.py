"""thinktwice_amd.evaluate on the GPU, on the generated dataset tree of tests/dataset_cases.py at final_dim = (128, 256), B = 2, as
tests/test_runner.py builds it: evaluate / validate(metrics=) / compare_modes / the runner's metrics / the command line, each
against the numpy restatement (tests/eval_ref.py) fed with the very `pred` tensors the models produced."""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dataset_cases as D  # noqa: E402
import eval_ref as E  # noqa: E402
from thinktwice_amd import calib  # noqa: E402

pytestmark = pytest.mark.gpu
HW, B, SEED = (128, 256), 2, 3
CONF = dict(calib.IDA_AUG_CONF, final_dim=HW, resize_lim=(0.56 * 128 / 448, 0.6255 * 128 / 448))     # test_runner.py's
TRAIN_TOWN, VAL_TOWN = "town03_00", "town01_00"            # 4 and 3 samples
L2_REL_LIMIT = 4 * 0.0                                     # tests/test_eval_metrics.py, profiles/eval_metrics.txt: 4 x the worst observed
BATCH_KEYS = ("waypoints", "action_mu", "action_sigma", "speed", "seg", "depth")
PRED_KEYS = ("pred_wp", "mu_branches", "sigma_branches", "pred_speed", "_seg_cl", "_depth_cl")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return D.write_tree(tmp_path_factory.mktemp("tree"))


def _loader(tree, town, train=False, rank=0, world=1):
    from thinktwice_amd import dataset
    from thinktwice_amd.loader import DeviceBatchLoader
    index = dataset.DatasetIndex(tree["metadata"], [town], D.CFG, root=tree["root"])
    return DeviceBatchLoader(index, D.CFG, CONF, batch_size=B, seed=SEED, prefetch=2, threads=8, train=train, rank=rank, world=world)


@pytest.fixture(scope="module")
def weights():
    from thinktwice_amd import model as tm, params
    _, cfg = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    return params.init_params(cfg, seed=0)


def _model(weights, dtype):
    from thinktwice_amd import model as tm
    m, _ = tm.build_thinktwice(final_dim=HW, dtype=dtype)
    m.load_state_dict({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in weights.items()})
    m.eval()
    return m


@pytest.fixture(scope="module")
def m3(weights):
    return _model(weights, "f32x3")


@pytest.fixture(scope="module")
def m32(weights):
    return _model(weights, torch.float32)


class Recorded:
    """While active, every forward_inference of `model` also leaves host copies of its outputs (and of the batch's labels)."""

    def __init__(self, model, keys=PRED_KEYS):
        self.model, self.keys, self.calls = model, keys, []

    def __enter__(self):
        inner = self.model.forward_inference

        def forward(batch, *a, **k):
            pred = inner(batch, *a, **k)
            self.calls.append(({n: batch[n].detach().float().cpu().numpy() for n in BATCH_KEYS},
                               {n: pred[n].detach().float().contiguous().cpu().numpy() for n in self.keys}))
            return pred
        self.model.forward_inference = forward
        return self

    def __exit__(self, *exc):
        del self.model.forward_inference


def _restated_raw(model, calls):
    """The accumulators of a MetricWindow over the recorded calls, by tests/eval_ref.py."""
    db, C = model.d_bound, 12
    Dn = int((db[1] - db[0]) / db[2])
    conf, bad, nf, depth, sums, counts = np.zeros((C, C), np.int64), 0, 0, [0] * 5, None, None
    for batch, pred in calls:
        c, b_, n_ = E.seg_confusion(pred["_seg_cl"], batch["seg"].reshape((-1,) + batch["seg"].shape[2:]), C, model.seg_downsample_factor)
        conf, bad, nf = conf + c, bad + b_, nf + n_
        d = E.depth_bins(pred["_depth_cl"], batch["depth"].reshape((-1,) + batch["depth"].shape[2:]), Dn, model.downsample_factor,
                         db[0], db[2])
        depth = [x + y for x, y in zip(depth, d)]
        sums, counts = E.decoder(pred["pred_wp"], pred["mu_branches"], pred["sigma_branches"], pred["pred_speed"], batch["waypoints"],
                                 batch["action_mu"], batch["action_sigma"], batch["speed"], sums, counts)
    return OrderedDict(seg_conf=conf.tolist(), seg_bad_label=bad, seg_nonfinite=nf, depth=depth, num_samples=counts[0],
                       dec_nonfinite=counts[1], dec_sums=sums.tolist(), d_step=float(db[2]))


def _same_raw(got, want, sums_exact=False):
    for k in ("seg_conf", "seg_bad_label", "seg_nonfinite", "depth", "num_samples", "dec_nonfinite"):
        assert got[k] == want[k], (k, got[k], want[k])
    g, w = np.asarray(got["dec_sums"]), np.asarray(want["dec_sums"])
    n = len(g)
    l1 = [i for i in range(n) if i == n - 1 or i % 8 >= 2]
    l2 = [i for i in range(n) if i != n - 1 and i % 8 < 2]
    if sums_exact:
        assert np.array_equal(g.view(np.int64), w.view(np.int64))
        return
    assert np.array_equal(g[l1].view(np.int64), w[l1].view(np.int64)), (g[l1], w[l1])
    rel = np.abs(g[l2] - w[l2]) / np.abs(w[l2])
    print(f"L2 sums against the restatement: worst relative error {rel.max():.3e} (limit {L2_REL_LIMIT:.3e})")
    assert rel.max() <= L2_REL_LIMIT


@pytest.fixture(scope="module")
def evaluated(tree, m3):
    """evaluate() of the f32x3 model over the validation town, with its forwards recorded."""
    from thinktwice_amd import evaluate
    val = _loader(tree, VAL_TOWN)
    with Recorded(m3) as rec:
        summary, raw = evaluate.evaluate(m3, val, raw=True)
    val.close()
    return dict(summary=summary, raw=raw, calls=rec.calls)


def test_evaluate_equals_the_restatement_on_the_same_outputs(m3, evaluated):
    from thinktwice_amd import evaluate
    raw, summary = evaluated["raw"], evaluated["summary"]
    assert [c[1]["pred_wp"].shape[0] for c in evaluated["calls"]] == [2, 1] and raw["num_samples"] == 3
    assert evaluated["calls"][0][1]["pred_wp"].shape[1] == 6 and len(raw["dec_sums"]) == 49
    want = _restated_raw(m3, evaluated["calls"])
    _same_raw(raw, want)
    cells = 3 * 4 * (HW[0] // 2) * (HW[1] // 2)
    assert sum(map(sum, raw["seg_conf"])) + raw["seg_bad_label"] + raw["seg_nonfinite"] <= cells
    assert sum(map(sum, raw["seg_conf"])) > 0 and raw["depth"][0] > 0 and raw["dec_nonfinite"] == 0
    names = evaluate.seg_class_names()
    restated = E.summarize(raw, names, 0.5)
    assert list(summary) == list(restated)
    for k in restated:
        assert summary[k] == restated[k] or (summary[k] != summary[k] and restated[k] != restated[k]), k
    assert all(np.isfinite(summary[f"wp_ade_{s}"]) and summary[f"wp_ade_{s}"] > 0 for s in range(6))
    assert 0.0 <= summary["seg_pixel_acc"] <= 1.0 and 0.0 <= summary["depth_within1"] <= 1.0


def test_add_does_not_wait_for_the_device(tree, m3):
    from thinktwice_amd import evaluate
    val = _loader(tree, VAL_TOWN)
    batch = next(iter(val))
    with torch.no_grad():
        pred = m3.forward_inference(batch)
    window = evaluate.window_for(m3)
    window.add(batch, pred)                                          # (first use: lazy initialisation may wait)
    torch.cuda.synchronize()
    live = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        window.add(batch, pred)
        pending = window.close()
        try:
            torch.ones(1, device="cuda").item()
        except RuntimeError:
            live = True                                              # the mode does catch a synchronising call on this build
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print(f"torch.cuda.set_sync_debug_mode('error') catches .item() on this build: {live}")
    val.close()
    assert pending.result()["num_samples"] == 2 * batch["speed"].shape[0]
    assert live, "set_sync_debug_mode('error') is inert on this build: MetricWindow.add's no-wait requirement was not exercised"


def test_validate_with_metrics_is_the_same_pass_and_the_same_metrics(tree, weights, evaluated):
    from thinktwice_amd import evaluate, model as tm
    from thinktwice_amd.runner import validate
    from thinktwice_amd.trainer import Trainer
    m, _ = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    trainer = Trainer(m, weights, lr=1e-4, frozen_bn=False)
    val = _loader(tree, VAL_TOWN)
    plain = validate(trainer, val)
    window = evaluate.window_for(trainer.model)
    both = validate(trainer, val, metrics=window)
    val.close()
    assert trainer.model.pred_observer is None
    flat = evaluate.scalar_metrics(evaluated["summary"])
    assert list(both) == list(plain)[:-2] + list(flat) + ["num_samples", "eval_iter_num"]
    for k in plain:                                                  # the loss means: bit for bit
        assert np.float64(plain[k]).view(np.int64) == np.float64(both[k]).view(np.int64), k
    for k, v in flat.items():                                        # the metrics: evaluate()'s on a model in the same mode
        assert both[k] == v or (both[k] != both[k] and v != v), (k, both[k], v)


def test_two_ranks_merged_equal_one_rank_in_every_integer(tree, m3):
    from thinktwice_amd import evaluate
    one = _loader(tree, TRAIN_TOWN)
    _, whole = evaluate.evaluate(m3, one, raw=True)
    one.close()
    parts = []
    for rank in (0, 1):
        ld = _loader(tree, TRAIN_TOWN, rank=rank, world=2)
        parts.append(evaluate.evaluate(m3, ld, raw=True)[1])
        ld.close()
    assert [p["num_samples"] + p["dec_nonfinite"] for p in parts] == [2, 2]
    merged = evaluate.merge_raw(parts)
    for k in ("seg_conf", "seg_bad_label", "seg_nonfinite", "depth", "num_samples", "dec_nonfinite"):
        assert merged[k] == whole[k], k
    assert whole["num_samples"] + whole["dec_nonfinite"] == 4


def test_compare_modes_of_a_model_with_itself_is_all_zeros(tree, m3):
    from thinktwice_amd import evaluate
    val = _loader(tree, VAL_TOWN)
    out = evaluate.compare_modes(m3, m3, val)
    val.close()
    assert list(out["outputs"]) == list(evaluate.OUTPUT_KEYS)
    for k, v in out["outputs"].items():
        assert v["max_abs_diff"] == 0.0 and v["rel"] == 0.0 and v["max_abs"] > 0.0 and v["nonfinite"] == 0, (k, v)
    assert out["wp_l2_max_mm"] == 0.0 and out["wp_l2_mean_mm"] == 0.0 and out["wp_points"] == 3 * 6 * 4
    assert out["seg_cells_differ"] == 0 and out["seg_cells"] == 3 * 4 * 64 * 128 and out["seg_differ_share"] == 0.0
    assert all(v == 0.0 or v != v for v in out["delta"].values()) and out["a"]["num_samples"] == 3


def test_compare_modes_equals_the_restatement(tree, m32, m3):
    """f32 against f32x3: the report is the restatement's over the two models' own outputs.  No bound is asserted at this size."""
    from thinktwice_amd import evaluate
    keys = tuple(evaluate.OUTPUT_KEYS) + ("_seg_cl",)
    val = _loader(tree, VAL_TOWN)
    with Recorded(m32, keys) as ra, Recorded(m3, keys) as rb:
        out = evaluate.compare_modes(m32, m3, val)
    val.close()
    assert len(ra.calls) == len(rb.calls) == 2
    for k in evaluate.OUTPUT_KEYS:
        d = [E.pair_deviation(a[1][k], b[1][k]) for a, b in zip(ra.calls, rb.calls)]
        got = out["outputs"][k]
        assert got["max_abs_diff"] == float(max(x[0] for x in d)) and got["max_abs"] == float(max(x[1] for x in d)), k
        assert got["nonfinite"] == sum(x[2] for x in d) and got["rel"] == got["max_abs_diff"] / got["max_abs"]
    ms, cnt = (0.0, 0.0), (0, 0)
    seg = [0, 0, 0]
    for a, b in zip(ra.calls, rb.calls):
        ms, cnt = E.pair_wp(a[1]["pred_wp"], b[1]["pred_wp"], ms, cnt)
        seg = [x + y for x, y in zip(seg, E.pair_seg(a[1]["_seg_cl"], b[1]["_seg_cl"], 12))]
    assert out["wp_points"] == cnt[0] == 72 and out["wp_nonfinite"] == 0
    assert abs(out["wp_l2_max_mm"] - ms[0] * 1e3) <= L2_REL_LIMIT * ms[0] * 1e3
    assert abs(out["wp_l2_mean_mm"] - ms[1] / 72 * 1e3) <= 2 * L2_REL_LIMIT * ms[1] / 72 * 1e3
    assert [out["seg_cells_differ"], out["seg_cells"], out["seg_cells_nonfinite"]] == seg
    print("compare_modes(f32, f32x3):", json.dumps({k: v["rel"] for k, v in out["outputs"].items()}), "wp mm", out["wp_l2_max_mm"],
          out["wp_l2_mean_mm"], "seg share", out["seg_differ_share"])
    assert set(out["delta"]) == set(evaluate.scalar_metrics(out["a"])) & set(evaluate.scalar_metrics(out["b"]))


def test_the_runner_logs_the_metrics_and_keeps_the_best_by_one(tree, weights, tmp_path):
    from thinktwice_amd import model as tm, ops
    from thinktwice_amd.runner import EpochRunner
    from thinktwice_amd.trainer import Trainer
    ops.DROPOUT_SEED[:] = [0x5EED, 0]
    m, _ = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    trainer = Trainer(m, weights, lr=1e-4, frozen_bn=False)
    train, val = _loader(tree, TRAIN_TOWN, train=True), _loader(tree, VAL_TOWN)
    work = str(tmp_path / "work")
    runner = EpochRunner(trainer, train, val, work_dir=work, max_epochs=1, log_interval=1, verbose=False, metrics=True,
                         save_best="wp_ade_5")
    logs = runner.run()
    train.close()
    val.close()
    assert sorted(os.listdir(work)) == ["best_wp_ade_5.pth", "epoch_1.pth", "latest.pth", "log.json"]
    line = [x for x in logs if x["mode"] == "val"][0]
    keys = list(line)
    assert keys.index("loss") < keys.index("wp_ade_0") < keys.index("seg_miou") < keys.index("depth_top1") < keys.index("num_samples")
    assert runner.best == line["wp_ade_5"] and np.isfinite(runner.best)
    ckpt = torch.load(os.path.join(work, "best_wp_ade_5.pth"), weights_only=False)
    assert ckpt["meta"]["runner"]["best"] == runner.best
    with open(os.path.join(work, "log.json")) as f:
        assert json.loads(f.readlines()[-1])["wp_ade_5"] == line["wp_ade_5"]


def test_the_command_line_writes_the_numbers_of_evaluate(tree, weights, evaluated, tmp_path):
    from thinktwice_amd import evaluate
    ckpt, out = str(tmp_path / "w.pth"), str(tmp_path / "metrics.json")
    torch.save({"state_dict": weights}, ckpt)
    evaluate.main(["--data-root", tree["root"], "--metadata", tree["metadata"], "--load-from", ckpt, "--dtype", "f32x3", "--towns",
                   VAL_TOWN, "--dev", "--batch-size", str(B), "--final-dim", str(HW[0]), str(HW[1]), "--seed", str(SEED), "--out", out])
    with open(out) as f:
        got = json.load(f, object_pairs_hook=OrderedDict)
    assert got["dtype"] == "f32x3" and got["towns"] == [VAL_TOWN] and got["world"] == 1
    want = json.loads(json.dumps(evaluate._jsonable(evaluated["summary"])), object_pairs_hook=OrderedDict)
    assert got["metrics"] == want
