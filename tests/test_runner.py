"""runner.EpochRunner / runner.validate / train.main on the GPU, on the generated dataset tree of tests/dataset_cases.py at
final_dim = (128, 256), B = 2, f32x3, frozen_bn=False: the training index is one town of 4 samples (an epoch is 2 iterations),
the validation index one town of 3 samples (batches of 2 + 1, so the weights matter).  One uninterrupted three-epoch run,
validated and checkpointed every epoch, is computed once; every comparison is of bits."""
import json
import os
import shutil
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dataset_cases as D  # noqa: E402
import logvars_ref as R  # noqa: E402
from thinktwice_amd import calib  # noqa: E402

pytestmark = pytest.mark.gpu
HW, B, SEED = (128, 256), 2, 3
CONF = dict(calib.IDA_AUG_CONF, final_dim=HW, resize_lim=(0.56 * 128 / 448, 0.6255 * 128 / 448))     # test_loader.py's
TRAIN_TOWN, VAL_TOWN = "town03_00", "town01_00"
EPOCHS = 3


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return D.write_tree(tmp_path_factory.mktemp("tree"))


def _loader(tree, town, train):
    from thinktwice_amd import dataset
    from thinktwice_amd.loader import DeviceBatchLoader
    index = dataset.DatasetIndex(tree["metadata"], [town], D.CFG, root=tree["root"])
    return DeviceBatchLoader(index, D.CFG, CONF, batch_size=B, seed=SEED, prefetch=2, threads=8, train=train)


def _objects(tree):
    """Identically seeded model, trainer and loaders; the dropout generator at its start."""
    from thinktwice_amd import model as tm, ops, params
    from thinktwice_amd.trainer import Trainer
    ops.DROPOUT_SEED[:] = [0x5EED, 0]
    m, cfg = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    trainer = Trainer(m, params.init_params(cfg, seed=0), lr=1e-4, frozen_bn=False)
    train, val = _loader(tree, TRAIN_TOWN, True), _loader(tree, VAL_TOWN, False)
    assert len(train) == 2 and len(val.index) == 3 and len(val) == 2
    return trainer, train, val, cfg


def _lines(work):
    with open(os.path.join(work, "log.json")) as f:
        return [json.loads(line, object_pairs_hook=OrderedDict) for line in f]


def _same(a, b, what=""):
    """Nested dicts / lists / tensors / numbers, bit for bit."""
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape, what
        assert torch.equal(a.cpu(), b.cpu()), what
    elif isinstance(a, dict):
        assert list(a) == list(b), what
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    elif isinstance(a, float):
        assert R.bits64(a) == R.bits64(b), (what, a, b)
    else:
        assert a == b, (what, a, b)


def _untimed(line):
    return OrderedDict((k, v) for k, v in line.items() if k != "time")


@pytest.fixture(scope="module")
def whole(tree, tmp_path_factory):
    """The uninterrupted run: 3 epochs of 2 iterations, a log line per iteration, validation and a checkpoint per epoch."""
    from thinktwice_amd.runner import EpochRunner
    work = str(tmp_path_factory.mktemp("whole"))
    trainer, train, val, cfg = _objects(tree)
    runner = EpochRunner(trainer, train, val, work_dir=work, max_epochs=EPOCHS, log_interval=1, verbose=False)
    runner.run()
    out = {"work": work, "lines": _lines(work), "state": trainer.state_dict(), "optimizer": trainer.optimizer_state_dict(),
           "trainer": trainer, "train": train, "val": val, "cfg": cfg}
    train.close()
    val.close()
    return out


def _names(line):
    return [k for k in line if k not in ("mode", "epoch", "iter", "lr", "time", "num_samples", "iterations", "skipped", "grad_norm")]


@pytest.fixture(scope="module")
def hand(tree):
    """Two epochs of `for batch in loader: trainer.step(batch)` on identically seeded objects, under the whole run's schedule:
    the log lines the runner would write (windows of one iteration: the mean is the value) and the final state."""
    trainer, train, val, _ = _objects(tree)
    val.close()
    trainer.set_schedule(EPOCHS * len(train), len(train))
    want = []
    for e in range(2):
        train.set_epoch(e)
        for i, batch in enumerate(train, 1):
            lr = trainer.current_lr()
            if e == 0 and i == 1:
                with pytest.raises(RuntimeError, match="between epochs"):    # the prefetched batches' draws are taken
                    train.state()
            out = trainer.step(batch)
            win = R.HostWindow(len(out["log_vars"]) + 1)
            win.add(list(out["log_vars"].values()) + [float(out["grad_norm"][0])], out["num_samples"])
            names = tuple(out["log_vars"]) + ("grad_norm",)
            line = OrderedDict(mode="train", epoch=e + 1, iter=i, lr=lr)
            line.update(R.window_means(names, win.flush()))
            want.append(line)
    train.close()
    return {"lines": want, "state": trainer.state_dict(), "optimizer": trainer.optimizer_state_dict()}


def test_the_run_equals_the_hand_loop(whole, hand):
    """Two epochs of the runner == the hand loop on identically seeded objects, bit for bit: every logged window (one iteration
    each) is the mean of that iteration's float log_vars, the state is epoch_2.pth's.  (Two executions of a training step give
    the same bits: the backward's scatters add in a fixed order, csrc/look_bwd.hip, csrc/glue_bwd.hip.)"""
    got = [_untimed(x) for x in whole["lines"] if x["mode"] == "train" and x["epoch"] <= 2]
    assert len(got) == len(hand["lines"]) == 4
    for g, w in zip(got, hand["lines"]):
        assert g["skipped"] == 0 and g["iterations"] == 1 and g["num_samples"] == B and len(g) == 4 + 25 + 3
        _same(dict(g), dict(w), f"epoch {w['epoch']} iteration {w['iter']}")
    ckpt = torch.load(os.path.join(whole["work"], "epoch_2.pth"), weights_only=False)
    _same(ckpt["state_dict"], hand["state"], "state_dict")
    _same(ckpt["optimizer"], hand["optimizer"], "optimizer")


@pytest.fixture(scope="module")
def resumed(tree, whole, tmp_path_factory):
    """Epochs [0, 1] are the whole run's epoch_2.pth; fresh objects, resume('auto'), epoch [2]."""
    from thinktwice_amd import ops
    from thinktwice_amd.runner import EpochRunner
    work = str(tmp_path_factory.mktemp("resumed"))
    shutil.copyfile(os.path.join(whole["work"], "epoch_2.pth"), os.path.join(work, "latest.pth"))     # the state after [0, 1]
    trainer, train, val, _ = _objects(tree)
    train.ida_sampler.sample(B, 4)                                      # fresh objects need not be in step: the state decides
    ops.DROPOUT_SEED[:] = [1, 99]
    runner = EpochRunner(trainer, train, val, work_dir=work, max_epochs=EPOCHS, log_interval=1, verbose=False)
    assert runner.resume("auto") == 2 and trainer.iteration == 4
    runner.run()
    train.close()
    val.close()
    return {"work": work, "lines": _lines(work), "state": trainer.state_dict(), "optimizer": trainer.optimizer_state_dict()}


def test_resume_continues_the_uninterrupted_run(whole, resumed):
    """Epochs [0, 1], fresh objects, resume('auto'), epoch [2] == the uninterrupted [0, 1, 2]: parameters, moments, running
    statistics, num_batches_tracked and epoch 3's log lines, bit for bit."""
    _same(whole["state"], resumed["state"], "state_dict")               # parameters, running statistics, num_batches_tracked
    _same(whole["optimizer"], resumed["optimizer"], "optimizer")        # moments, step counts, rates
    got, want = resumed["lines"], [x for x in whole["lines"] if x["epoch"] == 3]
    assert [x["mode"] for x in got] == ["train", "train", "val"] == [x["mode"] for x in want]
    for g, w in zip(got, want):
        _same(dict(_untimed(g)), dict(_untimed(w)), f"epoch 3 {w['mode']} line, iteration {w['iter']}")
    assert sorted(os.listdir(resumed["work"])) == ["epoch_3.pth", "latest.pth", "log.json"]
    ckpt = torch.load(os.path.join(resumed["work"], "latest.pth"), weights_only=False)
    assert ckpt["meta"]["epoch"] == 3 and ckpt["meta"]["iter"] == 6


def test_validation_is_the_reference_loop_and_leaves_the_trainer_alone(tree, whole):
    from thinktwice_amd import model as tm, ops
    from thinktwice_amd.runner import validate
    trainer, val = whole["trainer"], _loader(tree, VAL_TOWN, False)
    before = trainer.checkpoint(EPOCHS)
    counters = (trainer.iteration, trainer.epoch, trainer._bn_steps, list(ops.DROPOUT_SEED), trainer.opt.issued, trainer.model.training)
    got = validate(trainer, val)
    assert (trainer.iteration, trainer.epoch, trainer._bn_steps, list(ops.DROPOUT_SEED), trainer.opt.issued,
            trainer.model.training) == counters
    _same(before, trainer.checkpoint(EPOCHS), "checkpoint around validate()")
    # the literal loop of custom_multi_gpu_test on a fresh eval() model holding the trainer's weights
    fresh, _ = tm.build_thinktwice(final_dim=HW, dtype="f32x3")
    fresh.load_state_dict({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in trainer.state_dict().items()})
    fresh.eval()
    results, seen, sizes = OrderedDict(), 0.0, []
    for batch in val:
        with torch.no_grad():
            out = fresh.train_step(batch, None)
        for key, v in out["log_vars"].items():
            results[key] = results.get(key, 0.0) + v * out["num_samples"]
        seen += out["num_samples"]
        sizes.append(out["num_samples"])
    val.close()
    assert sizes == [2, 1] and got["num_samples"] == 3 and got["eval_iter_num"] == 2
    assert list(got)[:-2] == list(results)
    for key in results:
        assert R.bits64(got[key]) == R.bits64(results[key] / seen), (key, got[key], results[key] / seen)
    # the run's own validation line of the last epoch was taken at this very state
    line = [x for x in whole["lines"] if x["mode"] == "val"][-1]
    assert line["epoch"] == EPOCHS and all(R.bits64(line[k]) == R.bits64(got[k]) for k in results)
    # the next training step is the one that would have been taken without the validation
    train = _loader(tree, TRAIN_TOWN, True)
    train.set_epoch(0)
    batch = next(iter(train))
    train.close()
    first = trainer.step(batch)
    norm1, state1 = first["grad_norm"].clone(), trainer.checkpoint(EPOCHS)
    trainer.load_checkpoint(before)
    ops.DROPOUT_SEED[:] = counters[3]
    again = trainer.step(batch)                                          # no validation before this one
    _same(dict(first["log_vars"]), dict(again["log_vars"]), "log_vars of the step after validate()")
    _same(norm1, again["grad_norm"], "grad_norm of the step after validate()")
    _same(state1, trainer.checkpoint(EPOCHS), "state after the step after validate()")


class Poisoned:
    """A loader whose batches number `bad` (1-based, counted over the epochs) carry a NaN in a loss target, the Beta
    distribution's action_mu: the KL term's gradient reads it (a NaN waypoint or value target would not do: the smooth-L1
    gradient is a clamp of the difference, finite whatever the target), so the gradient norm is not finite."""

    def __init__(self, loader, bad):
        self.loader, self.bad, self.count = loader, set(bad), 0

    def __len__(self):
        return len(self.loader)

    def set_epoch(self, e):
        self.loader.set_epoch(e)

    def state(self):
        return self.loader.state()

    def __iter__(self):
        for batch in self.loader:
            self.count += 1
            if self.count in self.bad:
                batch = dict(batch)
                batch["action_mu"] = batch["action_mu"].clone()
                batch["action_mu"].view(-1)[0] = float("nan")
            yield batch


def test_non_finite_steps_stay_out_of_the_window_and_a_window_of_them_raises(tree, whole, tmp_path):
    from thinktwice_amd.runner import EpochRunner
    trainer, train, val, _ = _objects(tree)
    val.close()
    runner = EpochRunner(trainer, Poisoned(train, [2]), work_dir=str(tmp_path / "a"), max_epochs=1, log_interval=2, verbose=False)
    # (the schedule's length differs from the whole run's; during warm-up of the first epoch the rate does not depend on it)
    runner.run()
    (line,) = _lines(str(tmp_path / "a"))
    assert line["skipped"] == 1 and line["iterations"] == 1 and line["num_samples"] == B and line["iter"] == 2
    first = whole["lines"][0]                                            # the same first iteration, logged alone
    assert first["epoch"] == 1 and first["iter"] == 1
    names = _names(first)
    names = names + ["grad_norm"]
    assert len(names) == 25 and all(np.isfinite(line[k]) for k in names)
    for k in names:                                                      # the NaN iteration is absent from the means
        assert R.bits64(line[k]) == R.bits64(first[k]), (k, line[k], first[k])
    assert trainer.iteration == 1 and trainer.opt.steps == 1             # reconcile() counted the same iterations
    ckpt = torch.load(os.path.join(str(tmp_path / "a"), "epoch_1.pth"), weights_only=False)
    assert ckpt["meta"]["iter"] == 1
    again = EpochRunner(trainer, Poisoned(train, [1, 2]), work_dir=str(tmp_path / "b"), max_epochs=1, log_interval=2, verbose=False)
    with pytest.raises(FloatingPointError, match="non-finite"):
        again.run()
    train.close()


def test_the_entry_point_trains_an_epoch(tree, tmp_path):
    from thinktwice_amd import train
    work = str(tmp_path / "work")
    logs = train.main(["--data-root", tree["root"], "--metadata", tree["metadata"], "--work-dir", work, "--dev", "--epochs", "1",
                       "--batch-size", str(B), "--final-dim", str(HW[0]), str(HW[1]), "--log-interval", "1", "--seed", str(SEED)])
    assert sorted(os.listdir(work)) == ["epoch_1.pth", "latest.pth", "log.json"]
    lines = _lines(work)
    assert [x["mode"] for x in lines] == ["train", "train", "val"] and [dict(x) for x in lines] == [json.loads(json.dumps(x)) for x in logs]
    assert all(np.isfinite(x["loss"]) and x["epoch"] == 1 for x in lines) and lines[2]["num_samples"] == 3
    ckpt = torch.load(os.path.join(work, "latest.pth"), weights_only=False)
    assert ckpt["meta"]["epoch"] == 1 and ckpt["meta"]["iter"] == 2 and set(ckpt["meta"]["runner"]) == {"loader", "dropout_seed", "best"}
    assert ckpt["meta"]["runner"]["loader"][0]["photometric"]["reads"] == 2 * B
