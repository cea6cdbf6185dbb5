"""Gradient accumulation without a GPU: runner.accumulation_plan against an in-test restatement of mmcv's
GradientCumulativeOptimizerHook, and EpochRunner(cumulative_iters=k) on a fake trainer (the fakes of tests/test_runner_cpu.py,
with a step() that takes `window`): which (j, k) every step receives, when the held-back logged values are added and under which
gate, that a checkpoint is only asked for with no window open, and the command line."""
import os
import sys
import warnings

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_runner_cpu as C  # noqa: E402
from thinktwice_amd import runner  # noqa: E402


def _hook(n, k):
    """mmcv's hook over ONE epoch of n iterations, restated from its four quantities: -> [(updates, loss factor)] per iteration.
    (mmcv runs them over the run's max_iters; the runner applies the rule per epoch, see accumulation_plan.)"""
    divisible_iters = n // k * k
    remainder_iters = n - divisible_iters
    out = []
    for it in range(n):                                   # runner.iter before the increment, as after_train_iter sees it
        loss_factor = k if it < divisible_iters else remainder_iters
        every_n_iters = (it + 1) % k == 0
        is_last_iter = it + 1 == n
        out.append((every_n_iters or is_last_iter, loss_factor))
    return out


def test_the_plan_is_the_hooks_rule():
    for n in range(1, 41):
        for k in range(1, 9):
            plan = runner.accumulation_plan(n, k)
            assert len(plan) == n
            assert [(j == ke - 1, ke) for j, ke in plan] == _hook(n, k), (n, k)
            # every window counts 0 .. k_eff - 1 without a gap and ends the epoch closed
            expect = 0
            for j, ke in plan:
                assert j == expect and 1 <= ke <= k
                expect = 0 if j == ke - 1 else j + 1
            assert expect == 0
    assert runner.accumulation_plan(0, 3) == []
    with pytest.raises(ValueError):
        runner.accumulation_plan(5, 0)


class WindowTrainer(C.FakeTrainer):
    """FakeTrainer whose step() takes `window` and keeps the order rules of Trainer.step; `bad`: 1-based steps whose CLOSE
    reports a non-finite norm."""

    def __init__(self, bad=()):
        super().__init__(bad)
        self.windows, self.open, self.checkpoints_with_open_window = [], None, 0

    def step(self, batch, check_finite=True, device_log=False, window=None):
        assert device_log and not check_finite
        self.windows.append(window)
        if window is None:
            assert self.open is None
            out = super().step(batch, check_finite=check_finite, device_log=device_log)
            return out
        j, k = window
        assert (self.open is None and j == 0) or self.open == (j, k), (self.open, window)
        self.open = (j + 1, k) if j < k - 1 else None
        self.steps.append(batch["x"])
        self.iteration += 1
        v = float(batch["x"])
        out = dict(loss=v, log_vars=C.FakeLogVars([v, 0.5 * v, 1.5 * v]), num_samples=batch["n"], grad_norm=None, updated=False)
        if self.open is None:
            norm = float("nan") if len(self.steps) in self.bad else 1.0 + v
            if norm != norm:
                self.iteration -= k
            out.update(grad_norm=[norm, 1.0], updated=True)
        return out

    def checkpoint(self, epoch):
        self.checkpoints_with_open_window += self.open is not None
        return super().checkpoint(epoch)


class SpyWindow(C.FakeWindow):
    """Notes, per add, how many trainer steps had been taken and the gate it came with."""
    trainer, seen = None, None

    def add(self, log_vars, num_samples, gate=None, extra=None):
        SpyWindow.seen.append((len(SpyWindow.trainer.steps), log_vars.values[0], gate[0], extra["grad_norm"][0]))
        super().add(log_vars, num_samples, gate=gate, extra=extra)


def _run(tmp_path, n, k, bad=(), **kw):
    trainer = WindowTrainer(bad)
    SpyWindow.trainer, SpyWindow.seen = trainer, []
    args = dict(work_dir=str(tmp_path), max_epochs=1, log_interval=1, make_window=SpyWindow, verbose=False, cumulative_iters=k)
    args.update(kw)
    r = runner.EpochRunner(trainer, C.FakeLoader(n), **args)
    r.run()
    return r, trainer, C._lines(tmp_path)


def test_the_steps_get_their_windows_and_the_adds_wait_for_the_close(tmp_path):
    r, trainer, lines = _run(tmp_path, n=5, k=2)
    assert trainer.windows == [(0, 2), (1, 2), (0, 2), (1, 2), (0, 1)]
    # adds only at closes (after steps 2, 4, 5), in iteration order, every one under the gate of ITS window's close
    assert [(at, x) for at, x, _, _ in SpyWindow.seen] == [(2, 0.0), (2, 1.0), (4, 2.0), (4, 3.0), (5, 4.0)]
    assert [g for _, _, g, _ in SpyWindow.seen] == [2.0, 2.0, 4.0, 4.0, 5.0]
    assert [g for _, _, _, g in SpyWindow.seen] == [2.0, 2.0, 4.0, 4.0, 5.0]
    assert trainer.checkpoints_with_open_window == 0 and trainer.open is None
    assert os.path.exists(os.path.join(str(tmp_path), "epoch_1.pth"))
    # log_interval = 1: the closes due at iterations 1 and 3 wait for their accumulation windows; `iter` is the latest one due
    assert [(x["iter"], x["iterations"], x["num_samples"]) for x in lines] == [(2, 2, 4), (4, 2, 4), (5, 1, 2)]
    assert lines[0]["wp_loss"] == (0.0 + 1.0) * 2 / 4 and lines[0]["grad_norm"] == 2.0
    assert sum(x["iterations"] for x in lines) == 5 and all(x["skipped"] == 0 for x in lines)
    meta = torch.load(os.path.join(str(tmp_path), "latest.pth"), weights_only=False)["meta"]
    assert meta["runner"]["cumulative_iters"] == 2 and meta["iter"] == 5


def test_a_log_close_inside_an_accumulation_window_waits_for_it(tmp_path):
    r, trainer, lines = _run(tmp_path, n=6, k=2, log_interval=3)
    # due at 3 (inside the window of iterations 3, 4): written at 4 with what it holds; the next one holds 5, 6
    assert [(x["iter"], x["iterations"]) for x in lines] == [(3, 4), (6, 2)]
    assert lines[0]["lr"] == 1e-4 / 3


def test_a_skipped_window_adds_nothing_and_counts_its_length(tmp_path):
    r, trainer, lines = _run(tmp_path, n=5, k=2, bad=[2], log_interval=5, ignore_last=False)
    (line,) = lines
    assert line["skipped"] == 2 and line["iterations"] == 3 and line["num_samples"] == 6
    assert line["wp_loss"] == (2.0 + 3.0 + 4.0) * 2 / 6                     # iterations 1, 2 (x = 0, 1) are absent
    assert trainer.iteration == 3
    # a remainder window counts ITS length
    r, trainer, lines = _run(tmp_path / "b", n=5, k=2, bad=[5], log_interval=5, ignore_last=False)
    assert lines[0]["skipped"] == 1 and lines[0]["iterations"] == 4


def test_cumulative_iters_one_is_the_plain_loop(tmp_path):
    trainer = C.FakeTrainer()                                               # its step() takes no `window` at all
    r = runner.EpochRunner(trainer, C.FakeLoader(3), work_dir=str(tmp_path / "a"), max_epochs=1, log_interval=1,
                           make_window=C.FakeWindow, verbose=False, cumulative_iters=1)
    r.run()
    assert len(trainer.steps) == 3
    r, trainer, lines = _run(tmp_path / "b", n=3, k=1)
    assert trainer.windows == [None, None, None] and [(x["iter"], x["iterations"]) for x in lines] == [(1, 1), (2, 1), (3, 1)]
    meta = torch.load(os.path.join(str(tmp_path / "b"), "latest.pth"), weights_only=False)["meta"]
    assert set(meta["runner"]) == {"loader", "dropout_seed", "best"}        # k = 1 writes the checkpoint it always wrote
    with pytest.raises(ValueError):
        runner.EpochRunner(trainer, C.FakeLoader(3), work_dir=str(tmp_path / "c"), cumulative_iters=0)


def test_resume_accepts_another_k_with_one_warning(tmp_path):
    from thinktwice_amd import ops
    saved = list(ops.DROPOUT_SEED)
    try:
        _run(tmp_path, n=4, k=2)
        for k, warns in ((2, False), (4, True), (1, True)):
            r = runner.EpochRunner(WindowTrainer(), C.FakeLoader(4), work_dir=str(tmp_path), max_epochs=2, make_window=C.FakeWindow,
                                   verbose=False, cumulative_iters=k)
            with warnings.catch_warnings(record=True) as got:
                warnings.simplefilter("always")
                assert r.resume("auto") == 1
            assert len([w for w in got if "cumulative_iters" in str(w.message)]) == (1 if warns else 0), (k, [str(w.message) for w in got])
    finally:
        ops.DROPOUT_SEED[:] = saved


def test_command_line_takes_cumulative_iters():
    from thinktwice_amd import train
    conf = train.assemble(train.parse_args(["--data-root", "r", "--work-dir", "w", "--cumulative-iters", "4"]))
    assert conf["cumulative_iters"] == 4 and "cumulative_iters" not in conf["runner"]
    assert train.assemble(train.parse_args(["--data-root", "r", "--work-dir", "w"]))["cumulative_iters"] == 1
