"""runner.EpochRunner, the cross-rank merge, the loader's resume state and the command line, without a GPU: the runner runs on
a fake trainer, fake loaders and a host log window (tests/logvars_ref.HostWindow), so what is checked is the loop itself --
which iterations log, which epochs validate and checkpoint, what a checkpoint carries and what resume() restores."""
import json
import os
import sys
import warnings
from collections import OrderedDict
from contextlib import contextmanager

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import logvars_ref as R  # noqa: E402
from thinktwice_amd import runner  # noqa: E402

NAMES = ("wp_loss", "speed_offset", "loss")
KEYS = ("mode", "epoch", "iter", "lr", "grad_norm", "num_samples", "skipped", "time") + NAMES


class FakeLogVars:
    def __init__(self, values):
        self.names, self.values = NAMES, values


class FakePending:
    def __init__(self, res):
        self.res = res

    def ready(self):
        return True

    def result(self):
        return self.res


class FakeWindow:
    """logvars.LogWindow's interface on the host restatement."""

    def __init__(self):
        self.names, self.win, self.adds = None, None, 0

    def add(self, log_vars, num_samples, gate=None, extra=None):
        extra = extra or {}
        if self.names is None:
            self.names = tuple(log_vars.names) + tuple(extra)
            self.win = R.HostWindow(len(self.names))
        self.win.add(list(log_vars.values) + [v[0] for v in extra.values()], num_samples, None if gate is None else gate[0])
        self.adds += 1

    def close(self):
        self.adds = 0
        return FakePending(R.window_means(self.names, self.win.flush()))


class FakeModel:
    device, training = "cpu", False

    def __init__(self, trainer):
        self.trainer = trainer

    def train(self, mode=True):
        self.training = mode

    def eval(self):
        self.training = False

    def train_step(self, batch, optimizer=None, device_log=False):
        assert device_log and not self.training and not torch.is_grad_enabled()
        v = float(batch["x"]) + self.trainer.iteration
        return dict(loss=v, log_vars=FakeLogVars([v, 2.0 * v, 3.0 * v]), num_samples=batch["n"])


class FakeTrainer:
    def __init__(self, bad=()):
        self.model, self.buffers = FakeModel(self), {}
        self.iteration = self.epoch = 0
        self.schedule, self.steps, self.bad, self.loaded, self.evaluations = None, [], set(bad), None, 0

    def set_schedule(self, total, per_epoch):
        self.schedule = (total, per_epoch)

    def current_lr(self):
        return 1e-4 / (1 + self.iteration)

    def step(self, batch, check_finite=True, device_log=False):
        assert device_log and not check_finite
        self.steps.append(batch["x"])
        v = float(batch["x"])
        norm = float("nan") if len(self.steps) in self.bad else 1.0 + v
        if norm == norm:
            self.iteration += 1
        return dict(loss=v, log_vars=FakeLogVars([v, 0.5 * v, 1.5 * v]), num_samples=batch["n"], grad_norm=[norm, 1.0])

    def reconcile(self):
        return 0

    @contextmanager
    def evaluating(self):
        self.evaluations += 1
        yield self.model

    def checkpoint(self, epoch):
        return {"meta": {"epoch": epoch, "iter": self.iteration}, "state_dict": {"w": torch.full((2,), float(self.iteration))},
                "optimizer": {}}

    def load_checkpoint(self, ckpt):
        self.loaded = ckpt
        self.epoch, self.iteration = ckpt["meta"]["epoch"], ckpt["meta"]["iter"]


class FakeLoader:
    def __init__(self, n, sizes=None):
        self.n, self.sizes, self.epoch, self.draws = n, sizes or [2] * n, None, 0

    def __len__(self):
        return self.n

    def set_epoch(self, e):
        self.epoch = e

    def __iter__(self):
        for k in range(self.n):
            self.draws += 1
            yield {"x": 10 * (self.epoch or 0) + k, "n": self.sizes[k]}

    def state(self):
        return {"draws": self.draws}

    def load_state(self, s):
        self.draws = s["draws"]


def _runner(tmp_path, n=7, trainer=None, **kw):
    trainer = trainer or FakeTrainer()
    args = dict(work_dir=str(tmp_path), max_epochs=1, log_interval=1, make_window=FakeWindow, verbose=False)
    args.update(kw)
    return runner.EpochRunner(trainer, FakeLoader(n), **args), trainer


def _lines(tmp_path):
    with open(os.path.join(str(tmp_path), "log.json")) as f:
        return [json.loads(line) for line in f]


@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("ignore_last", [True, False])
def test_which_iterations_close_a_window(tmp_path, interval, ignore_last):
    want = {(1, True): [1, 2, 3, 4, 5, 6, 7], (1, False): [1, 2, 3, 4, 5, 6, 7], (3, True): [3, 6], (3, False): [3, 6, 7]}
    assert R.log_schedule_ref(7, interval, ignore_last) == want[interval, ignore_last]
    assert runner.log_schedule(7, interval, ignore_last) == want[interval, ignore_last]
    r, trainer = _runner(tmp_path, log_interval=interval, ignore_last=ignore_last, max_epochs=2)
    r.run()
    assert trainer.schedule == (14, 7) and len(trainer.steps) == 14
    lines = [x for x in _lines(tmp_path) if x["mode"] == "train"]
    assert [(x["epoch"], x["iter"]) for x in lines] == [(e, i) for e in (1, 2) for i in want[interval, ignore_last]]
    # a window holds exactly the iterations since the previous close of ITS epoch: nothing leaks from a dropped tail
    for x in lines:
        k = want[interval, ignore_last].index(x["iter"])
        first = want[interval, ignore_last][k - 1] + 1 if k else 1
        xs = [10.0 * (x["epoch"] - 1) + (i - 1) for i in range(first, x["iter"] + 1)]
        assert x["iterations"] == len(xs) and x["num_samples"] == 2 * len(xs) and x["skipped"] == 0
        assert x["wp_loss"] == sum(v * 2.0 for v in xs) / (2.0 * len(xs))
        assert x["grad_norm"] == sum((1.0 + v) * 2.0 for v in xs) / (2.0 * len(xs))


def test_log_lines_parse_and_carry_the_keys(tmp_path):
    r, _ = _runner(tmp_path, n=3, val_loader=FakeLoader(2, sizes=[2, 1]))
    logs = r.run()
    lines = _lines(tmp_path)
    assert lines == [json.loads(json.dumps(x)) for x in logs] and [x["mode"] for x in lines] == ["train"] * 3 + ["val"]
    for x in lines[:3]:
        assert set(KEYS) <= set(x), sorted(set(KEYS) - set(x))
        assert x["epoch"] == 1 and x["time"] >= 0 and x["lr"] == 1e-4 / x["iter"]
    val = lines[3]
    assert val["epoch"] == 1 and val["eval_iter_num"] == 2 and val["num_samples"] == 3 and set(NAMES) <= set(val)
    # the weights matter: batches of 2 and 1 samples (x = 0 and 1, trainer.iteration = 3)
    assert val["wp_loss"] == ((0 + 3.0) * 2 + (1 + 3.0) * 1) / 3.0


def test_a_window_of_skipped_steps_only_raises_and_a_skipped_step_stays_out_of_the_mean(tmp_path):
    r, _ = _runner(tmp_path / "a", n=4, log_interval=2, trainer=FakeTrainer(bad=[2]))
    r.run()
    first = _lines(tmp_path / "a")[0]
    assert first["skipped"] == 1 and first["iterations"] == 1 and first["num_samples"] == 2 and first["wp_loss"] == 0.0
    r, _ = _runner(tmp_path / "b", n=4, log_interval=2, trainer=FakeTrainer(bad=[3, 4]))
    with pytest.raises(FloatingPointError, match="non-finite"):
        r.run()


@pytest.mark.parametrize("interval", [1, 2])
def test_which_epochs_validate_and_checkpoint(tmp_path, interval):
    r, trainer = _runner(tmp_path, n=2, max_epochs=4, val_loader=FakeLoader(2), eval_interval=interval, ckpt_interval=interval,
                         save_best="wp_loss")
    r.run()
    epochs = [e for e in range(1, 5) if e % interval == 0]
    assert [x["epoch"] for x in _lines(tmp_path) if x["mode"] == "val"] == epochs and trainer.evaluations == len(epochs)
    files = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith(".pth"))
    assert files == sorted([f"epoch_{e}.pth" for e in epochs] + ["latest.pth", "best_wp_loss.pth"])
    load = lambda name: torch.load(os.path.join(str(tmp_path), name), weights_only=False)       # noqa: E731
    latest, last = load("latest.pth"), load("epoch_4.pth")
    assert latest["meta"] == last["meta"] and latest["meta"]["epoch"] == 4 and torch.equal(latest["state_dict"]["w"], last["state_dict"]["w"])
    # the fake's validation value grows with trainer.iteration: the first validated epoch is the best one, lower is better
    best = load("best_wp_loss.pth")
    assert best["meta"]["epoch"] == epochs[0] and r.best == [x for x in _lines(tmp_path) if x["mode"] == "val"][0]["wp_loss"]
    assert latest["meta"]["runner"]["best"] == r.best


def test_resume_auto_picks_the_epoch_and_restores_the_runner_state(tmp_path):
    from thinktwice_amd import ops
    saved = list(ops.DROPOUT_SEED)
    try:
        ops.DROPOUT_SEED[:] = [0x5EED, 7]
        r, trainer = _runner(tmp_path, n=2, max_epochs=2)
        r.run()
        meta = torch.load(os.path.join(str(tmp_path), "latest.pth"), weights_only=False)["meta"]
        assert meta["epoch"] == 2 and meta["runner"]["loader"] == [{"draws": 4}] and meta["runner"]["dropout_seed"] == [0x5EED, 7]
        ops.DROPOUT_SEED[:] = [1, 2]
        r2, t2 = _runner(tmp_path, n=2, max_epochs=3)
        assert r2.resume("auto") == 2
        assert t2.loaded["meta"]["iter"] == 4 and r2.train_loader.draws == 4 and list(ops.DROPOUT_SEED) == [0x5EED, 7]
        r2.run()
        assert t2.steps == [20, 21] and r2.train_loader.epoch == 2            # epoch index 2 only
        assert [x["epoch"] for x in _lines(tmp_path)] == [1, 1, 2, 2, 3, 3]
        # nothing to resume from: the run starts fresh
        r3, _ = _runner(tmp_path / "empty", n=2)
        assert r3.resume("auto") is None and r3.epoch == 0
        # a reference (mmcv) checkpoint has no meta['runner']: it resumes, with a warning
        path = os.path.join(str(tmp_path), "mmcv.pth")
        torch.save({"meta": {"epoch": 1, "iter": 2}, "state_dict": {}, "optimizer": {}}, path)
        r4, t4 = _runner(tmp_path / "ref", n=2, max_epochs=2)
        with pytest.warns(UserWarning, match="augmentation"):
            assert r4.resume(path) == 1
        assert t4.iteration == 2 and r4.train_loader.draws == 0
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert r2.resume(os.path.join(str(tmp_path), "epoch_1.pth")) == 1
    finally:
        ops.DROPOUT_SEED[:] = saved


@pytest.mark.parametrize("ranks", [1, 2, 3])
def test_the_rank_merge_is_the_references(ranks):
    rng = np.random.default_rng(5 + ranks)
    counts = [3.0, 8.0, 5.0][:ranks]
    parts = [OrderedDict((k, float(rng.normal() * 10.0 ** int(rng.integers(-3, 4)))) for k in NAMES) for _ in range(ranks)]
    want = R.merge_ref([{k: (v, n) for k, v in p.items()} for p, n in zip(parts, counts)])
    got = runner.merge_ranks(list(zip(parts, counts)))
    assert list(got) == list(NAMES)
    for k in NAMES:
        assert R.bits64(got[k]) == R.bits64(want[k]), (k, got[k], want[k])
    if ranks == 1:
        for k in NAMES:                                  # mean * n / n need not be the mean: the reference's arithmetic is kept
            assert got[k] == parts[0][k] * 3.0 / 3.0
    # a rank whose share of the validation set is empty adds nothing
    more = runner.merge_ranks(list(zip(parts, counts)) + [(OrderedDict((k, float("nan")) for k in NAMES), 0)])
    assert all(R.bits64(more[k]) == R.bits64(got[k]) for k in NAMES)


def test_sampler_state_round_trip_draws_identical_sequences():
    from thinktwice_amd import calib, loader, photometric, preprocess
    rs = lambda k: np.random.RandomState([3, 0, k])                                # noqa: E731
    conf = dict(calib.IDA_AUG_CONF)
    a_ida, a_pho = preprocess.IdaSampler(conf, rs(0)), photometric.PhotometricSampler(2, rs(1))
    for _ in range(3):                                                             # an "epoch" of draws
        a_ida.sample(2, 4)
        a_pho.sample(2)
    state = loader.sampler_state(a_ida, a_pho)
    state = json.loads(json.dumps(state))                                          # plain data: survives a checkpoint
    b_ida, b_pho = preprocess.IdaSampler(conf, rs(7)), photometric.PhotometricSampler(2, rs(8))
    loader.load_sampler_state(b_ida, b_pho, state)
    assert b_pho.reads == a_pho.reads == 6
    for _ in range(3):
        assert a_ida.sample(2, 4) == b_ida.sample(2, 4)
        assert a_pho.sample(2) == b_pho.sample(2)
    assert loader.sampler_state(None, None) == {"ida": None, "photometric": None}
    with pytest.raises(ValueError, match="photometric"):
        loader.load_sampler_state(b_ida, None, state)


def test_command_line_parsing_and_config_assembly():
    from thinktwice_amd import data_config as dc, train
    args = train.parse_args(["--data-root", "/d/work", "--work-dir", "/w", "--dev", "--final-dim", "128", "256", "--batch-size", "2",
                             "--epochs", "3", "--lr", "3e-5", "--dtype", "f32", "--frozen-bn", "--no-augment", "--resume", "auto",
                             "--log-interval", "5", "--load-from", "x.pth"])
    conf = train.assemble(args)
    cfg = conf["cfg"]
    assert cfg["train_town"] == ["town01_00"] and cfg["val_town"] == ["town01_00"] and cfg["max_sample_per_town"]["town10"] == 10
    assert cfg["seg_label_idxs"] == [1, 4, 5, 6, 7, 8, 10, 12, 18] and cfg["history_query_index_lis"] == [-1, 0] and cfg["pred_len"] == 4
    assert cfg["camera_names"] == ["rgb_front", "rgb_left", "rgb_right", "rgb_back"] and cfg["is_local"]
    assert conf["ida_aug_conf"]["final_dim"] == (128, 256)
    assert conf["ida_aug_conf"]["resize_lim"] == (0.56 * 128 / 448, 0.6255 * 128 / 448) and conf["overrides"] == {"final_dim": (128, 256)}
    assert conf["trainer"] == dict(lr=3e-5, frozen_bn=True) and conf["loader"] == dict(batch_size=2, seed=0, augment=False)
    assert conf["runner"] == dict(work_dir="/w", max_epochs=3, log_interval=5, ckpt_interval=1, eval_interval=1)
    assert conf["metadata"] == os.path.join("/d/work", "..", "dataset", "dataset_metadata.pkl") and args.resume == "auto"
    # the defaults are the reference's job: the TCP split, 60 epochs, 8 per GPU, 1e-4, full size
    full = train.assemble(train.parse_args(["--data-root", "r", "--work-dir", "w"]))
    assert full["runner"]["max_epochs"] == 60 and full["loader"]["batch_size"] == 8 and full["trainer"]["lr"] == 1e-4
    assert full["overrides"] == {} and full["ida_aug_conf"]["final_dim"] == (448, 896) and full["ida_aug_conf"]["resize_lim"] == (0.56, 0.6255)
    assert len(full["cfg"]["train_town"]) == 4 * 13 and full["cfg"]["train_town"][:2] == ["town01_val", "town01_00"]
    assert full["cfg"]["val_town"][13] == "town05_val" and full["cfg"]["max_sample_per_town"]["town03"] == 42771
    assert len(dc.FULL_TRAIN) == 8 * 12 and dc.FULL_VAL[-1] == "town10_val"
    with pytest.raises(SystemExit):
        train.parse_args(["--work-dir", "w"])
