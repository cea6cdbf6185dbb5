"""A whole training job around `trainer.Trainer`: epochs, windowed logging, validation, checkpoints, resume -- what the
reference gets from train.py -> mmcv's EpochBasedRunner with its LoggerHook, CheckpointHook and the DistEvalHook of
core/evaluation/eval_hooks.py:116-152.  There is no hook system: `EpochRunner.run()` is one loop, and inside an epoch it adds no
host synchronisation of its own -- the logged values stay on the device (logvars.LogWindow) and a closed window is written when
its copy has arrived.

    runner = EpochRunner(trainer, train_loader, val_loader, work_dir="work", max_epochs=60)
    runner.resume("auto")               # continues from work/latest.pth if there is one
    runner.run()

Unpinned conventions (mmcv is not installed; these are owned by this module): `ignore_last=True` drops an epoch's incomplete
last window (mmcv LoggerHook's default, from memory), and the line format of log.json / the text line (`EpochRunner._write`).
"""
import collections
import contextlib
import json
import os
import shutil
import time
import warnings
from collections import OrderedDict

import torch


def log_schedule(iters_per_epoch, log_interval, ignore_last=True):
    """The 1-based inner iterations of an epoch after which a log window is closed AND written: every `log_interval`-th, and
    the last one too unless `ignore_last` (then an incomplete last window is dropped)."""
    out = [i for i in range(1, iters_per_epoch + 1) if i % log_interval == 0]
    if not ignore_last and iters_per_epoch > 0 and iters_per_epoch % log_interval != 0:
        out.append(iters_per_epoch)
    return out


def accumulation_plan(n_iters, k):
    """[(j, k_eff)] for the `n_iters` iterations of one epoch under gradient accumulation over `k`: iteration i is micro-step j
    of a window of k_eff, which updates at j == k_eff - 1.  mmcv's GradientCumulativeOptimizerHook restated (mmcv is not
    installed where this is built, so the rule is owned here): divisible_iters = n // k * k iterations form full windows with
    loss factor k; the n % k iterations after them form ONE short window whose loss factor is its own length, closed by the
    last iteration.  EpochRunner applies the plan per epoch (n = len(train_loader)): a window never spans an epoch boundary,
    where mmcv counts over the run's global iteration -- the two coincide when len(loader) % k == 0."""
    n_iters, k = int(n_iters), int(k)
    if n_iters < 0 or k < 1:
        raise ValueError(f"accumulation_plan: n_iters {n_iters} >= 0 and k {k} >= 1")
    divisible = n_iters // k * k
    return [(i % k, k) if i < divisible else (i - divisible, n_iters - divisible) for i in range(n_iters)]


def merge_ranks(parts):
    """collect_results_cpu's merge (eval_tool.py:146-160) over `parts` = [(means of rank r, samples of rank r)] in rank
    order: per name sum_r mean_r * n_r / sum_r n_r, Python floats.  A rank that saw no sample contributes nothing."""
    results, counts = OrderedDict(), {}
    for means, n in parts:
        if not n:
            continue
        for key, mean in means.items():
            if key not in results:
                results[key], counts[key] = 0.0, 0.0
            results[key] += mean * n
            counts[key] += n
    for key in results:
        results[key] /= counts[key]
    return results


def _dist(dist):
    if dist is None:
        import torch.distributed as td
        dist = td if (td.is_available() and td.is_initialized()) else None
    return dist


def is_better(value, best, rule="less"):
    """The `save_best` rule: `less` keeps the lowest value (a loss, an error in metres), `greater` the highest (seg_miou, an
    accuracy).  The first value is the best so far; a NaN never beats a value."""
    if rule not in ("less", "greater"):
        raise ValueError(f"save_best_rule is 'less' or 'greater', not {rule!r}")
    return best is None or (value < best if rule == "less" else value > best)


def parse_save_best(spec):
    """`NAME[:greater|:less]` of train.py's --save-best -> (name, rule)."""
    name, _, rule = str(spec).partition(":")
    rule = rule or "less"
    if not name or rule not in ("less", "greater"):
        raise ValueError(f"--save-best takes NAME[:greater|:less], not {spec!r}")
    return name, rule


def validate(target, loader, dist=None, window=None, metrics=None):
    """custom_multi_gpu_test (eval_tool.py:71-116) restated: the model under eval() and no_grad, `train_step` -- losses
    included, the reference evaluates forward_train too -- on every batch of `loader`, each batch's
    `log_vars` weighted by its size; ONE read at the end.  `target`: a Trainer (validated through `Trainer.evaluating()`) or a
    model.  Per rank the device window holds the reference's `results[k] += float(v) * batch_size` in f64, divided by the
    sample count when read; across ranks `merge_ranks` over one all_gather of (means, n) -- every rank returns the merged
    result.  Before a distributed validation rank 0's BatchNorm running statistics are broadcast (eval_hooks.py:123-129).
    `metrics`: an evaluate.MetricWindow filled from the SAME forwards through the model's `pred_observer` (no second pass, no
    host synchronisation per batch); its scalar metrics (evaluate.scalar_metrics, merged over the ranks) follow the loss means.
    -> OrderedDict: a mean per name, the metrics if asked for, then `num_samples` and `eval_iter_num` (this rank's batches)."""
    from . import logvars
    dist = _dist(dist)
    is_trainer = hasattr(target, "evaluating")
    model = target.model if is_trainer else target
    if dist is not None and dist.get_world_size() > 1 and is_trainer:
        for k in sorted(target.buffers):
            dist.broadcast(target.buffers[k], 0)
    if window is None:
        window = logvars.LogWindow(model.device)
    iters = 0
    if metrics is not None:
        model.pred_observer = metrics.add
    try:
        with (target.evaluating() if is_trainer else _eval_mode(model)), torch.no_grad():
            for batch in loader:
                out = model.train_step(batch, None, device_log=True)
                window.add(out["log_vars"], out["num_samples"])
                iters += 1
    finally:
        if metrics is not None:
            model.pred_observer = None
    if iters == 0:
        raise ValueError("validate: the loader gave no batch")
    res = window.close().result()
    n = res["num_samples"]
    means = OrderedDict((k, v) for k, v in res.items() if k not in logvars.COUNTERS)
    if dist is not None and dist.get_world_size() > 1:
        mine = torch.tensor(list(means.values()) + [float(n)], dtype=torch.float64,
                            device=model.device if dist.get_backend() != "gloo" else "cpu")
        parts = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, mine)
        parts = [p.tolist() for p in parts]
        means = merge_ranks([(OrderedDict(zip(means, p[:-1])), p[-1]) for p in parts])
        n = int(sum(p[-1] for p in parts))
    if metrics is not None:
        from . import evaluate
        means.update(evaluate.scalar_metrics(metrics.summarize(metrics.merge_ranks(metrics.close().result(), dist))))
    means["num_samples"], means["eval_iter_num"] = n, iters
    return means


@contextlib.contextmanager
def _eval_mode(model):
    was = model.training
    model.eval()
    try:
        yield model
    finally:
        model.train(was)


class EpochRunner:
    """See the module text.  `trainer`: a trainer.Trainer; the loaders: loader.DeviceBatchLoader (train=True / False) -- anything
    with __len__, __iter__, set_epoch and, for a bit-identical resume, state() / load_state().  `save_best`: a logged name;
    the checkpoint of the epoch with the LOWEST validation mean of it is kept as best_{name}.pth (`save_best_rule="greater"`: the
    highest, for seg_miou and the like).  `metrics=True`: the validation pass also fills an evaluate.MetricWindow from the same
    forwards; the task metrics join the validation line after the loss means and `save_best` may name one.  `make_window`: the factory of
    the log windows (default: logvars.LogWindow on the model's device).  `cumulative_iters` = k > 1: gradient accumulation, one
    optimizer update per window of k iterations (`accumulation_plan`, per epoch; the trainer's step(window=...)); 1: plain
    steps, the trainer's step() without a window.  The logged values of a window's micro-steps are held back (on the device) and
    added at its close, all gated by that close's gradient norm: a skipped window adds nothing to the means and counts its
    length as skipped.  `log_interval` and a line's `iter` count micro-iterations; a log window whose turn comes inside an
    accumulation window closes once that window's adds are issued, and its `iterations` says what it holds."""

    def __init__(self, trainer, train_loader, val_loader=None, work_dir="work_dir", max_epochs=1, log_interval=100,
                 ckpt_interval=1, eval_interval=1, ignore_last=True, save_best=None, dist=None, make_window=None, verbose=True,
                 cumulative_iters=1, metrics=False, save_best_rule="less"):
        if save_best_rule not in ("less", "greater"):
            raise ValueError(f"EpochRunner: save_best_rule is 'less' or 'greater', not {save_best_rule!r}")
        self.metrics, self.save_best_rule = bool(metrics), save_best_rule
        if min(int(max_epochs), int(log_interval), int(ckpt_interval), int(eval_interval), int(cumulative_iters)) < 1:
            raise ValueError("EpochRunner: max_epochs, the intervals and cumulative_iters are >= 1")
        self.cumulative_iters = int(cumulative_iters)
        self.trainer, self.train_loader, self.val_loader = trainer, train_loader, val_loader
        self.work_dir, self.max_epochs, self.log_interval = str(work_dir), int(max_epochs), int(log_interval)
        self.ckpt_interval, self.eval_interval, self.ignore_last = int(ckpt_interval), int(eval_interval), bool(ignore_last)
        self.save_best, self.verbose = save_best, verbose
        self.dist = _dist(dist)
        self.rank = self.dist.get_rank() if self.dist is not None else 0
        self.world = self.dist.get_world_size() if self.dist is not None else 1
        if make_window is None:
            from . import logvars
            make_window = lambda: logvars.LogWindow(trainer.model.device)      # noqa: E731
        self.make_window = make_window
        self.window = None
        self.epoch = 0                   # epochs completed
        self.best = None                 # best validation value of `save_best` so far (lowest, or highest under "greater")
        self.logs = []                   # every line written, as dicts (all ranks)
        os.makedirs(self.work_dir, exist_ok=True)

    # ------------------------------------------------------------------------------------------------------- logging
    def _write(self, line):
        """One log: a JSON line in work_dir/log.json and a text line, both by rank 0.  The format is this function's."""
        self.logs.append(line)
        if self.rank != 0:
            return
        with open(os.path.join(self.work_dir, "log.json"), "a") as f:
            f.write(json.dumps(line) + "\n")
        if self.verbose:
            skip = ("mode", "epoch", "iter")
            body = ", ".join(f"{k}: {v:.4e}" if isinstance(v, float) else f"{k}: {v}" for k, v in line.items() if k not in skip)
            print(f"Epoch({line['mode']}) [{line['epoch']}][{line['iter']}/{len(self.train_loader)}]  {body}", flush=True)

    def _write_window(self, pending, head):
        from .logvars import COUNTERS
        res = pending.result()
        if res["iterations"] == 0:
            raise FloatingPointError(f"EpochRunner: every step of the log window ending at epoch {head['epoch']}, iteration "
                                     f"{head['iter']} had a non-finite gradient norm ({res['skipped']} skipped updates)")
        line = OrderedDict(head)
        line.update((k, v) for k, v in res.items() if k not in COUNTERS)
        line["num_samples"], line["iterations"], line["skipped"] = res["num_samples"], res["iterations"], res["skipped"]
        line["time"] = line.pop("time")
        self._write(line)

    # ----------------------------------------------------------------------------------------------------- one epoch
    def _train_epoch(self, e):
        trainer, loader = self.trainer, self.train_loader
        n = len(loader)
        closes = set(log_schedule(n, self.log_interval, self.ignore_last))
        if self.window is None:
            self.window = self.make_window()
        window, pending = self.window, collections.deque()
        loader.set_epoch(e)
        t_last, i_last = time.perf_counter(), 0
        plan = accumulation_plan(n, self.cumulative_iters) if self.cumulative_iters > 1 else None
        held, due = [], None         # an open accumulation window's logged values; the log close whose turn has come: (iter, lr)
        for i, batch in enumerate(loader, 1):
            while pending and pending[0][0].ready():                  # non-blocking: written when the copy has arrived
                self._write_window(*pending.popleft())
            lr = trainer.current_lr()
            if i in closes:
                due = (i, lr)
            if plan is None:
                out = trainer.step(batch, check_finite=False, device_log=True)
            else:
                out = trainer.step(batch, check_finite=False, device_log=True, window=plan[i - 1])
                if not out["updated"]:
                    held.append((out["log_vars"], out["num_samples"]))
                    continue
                for log_vars, num in held:                            # the window's earlier micro-steps, under ITS gate
                    window.add(log_vars, num, gate=out["grad_norm"], extra={"grad_norm": out["grad_norm"]})
                held = []
            window.add(out["log_vars"], out["num_samples"], gate=out["grad_norm"], extra={"grad_norm": out["grad_norm"]})
            if due is not None:
                now = time.perf_counter()
                head = OrderedDict(mode="train", epoch=e + 1, iter=due[0], lr=due[1], time=(now - t_last) / (i - i_last))
                pending.append((window.close(), head))
                t_last, i_last, due = now, i, None
        if window.adds:
            window.close()                                            # ignore_last: the incomplete window is dropped
        while pending:
            self._write_window(*pending.popleft())

    # ---------------------------------------------------------------------------------------------------- checkpoints
    def _runner_meta(self):
        from . import ops
        state = self.train_loader.state() if hasattr(self.train_loader, "state") else None
        states = [state]
        if self.world > 1:                                            # every rank draws its own augmentation stream
            states = [None] * self.world
            self.dist.all_gather_object(states, state)
        meta = {"loader": states, "dropout_seed": list(ops.DROPOUT_SEED), "best": self.best}
        if self.cumulative_iters > 1:                                 # (absent: 1, what every earlier checkpoint is)
            meta["cumulative_iters"] = self.cumulative_iters
        return meta

    def _save(self, ckpt, name):
        path = os.path.join(self.work_dir, name)
        torch.save(ckpt, path + ".tmp")
        os.replace(path + ".tmp", path)
        return path

    def run(self):
        trainer, n = self.trainer, len(self.train_loader)
        trainer.set_schedule(self.max_epochs * n, n)
        for e in range(self.epoch, self.max_epochs):
            self._train_epoch(e)
            trainer.reconcile()
            val = None
            if self.val_loader is not None and (e + 1) % self.eval_interval == 0:
                lr = trainer.current_lr()
                mwin = None
                if self.metrics:
                    from . import evaluate
                    mwin = evaluate.window_for(trainer.model)
                val = validate(trainer, self.val_loader, dist=self.dist, window=self.make_window(), metrics=mwin)
                line = OrderedDict(mode="val", epoch=e + 1, iter=n, lr=lr)
                line.update(val)
                self._write(line)
            better = (val is not None and self.save_best is not None and self.save_best in val
                      and is_better(val[self.save_best], self.best, self.save_best_rule))
            if better:
                self.best = val[self.save_best]
            if (e + 1) % self.ckpt_interval == 0 or better:
                meta = self._runner_meta()                            # (collective: every rank)
                if self.rank == 0:
                    ckpt = trainer.checkpoint(e + 1)
                    ckpt["meta"]["runner"] = meta
                    if (e + 1) % self.ckpt_interval == 0:
                        path = self._save(ckpt, f"epoch_{e + 1}.pth")
                        shutil.copyfile(path, os.path.join(self.work_dir, "latest.pth.tmp"))
                        os.replace(os.path.join(self.work_dir, "latest.pth.tmp"), os.path.join(self.work_dir, "latest.pth"))
                    if better:
                        self._save(ckpt, f"best_{self.save_best}.pth")
            self.epoch = e + 1
        return self.logs

    def resume(self, path="auto"):
        """Continue from a checkpoint: `auto` is work_dir/latest.pth (none there: returns None, the run starts fresh), else
        a file.  The trainer loads weights, optimizer state and counters; meta['runner'] brings back the loader's augmentation
        streams, the dropout generator's counter and the best validation value, so that the continued run is the
        uninterrupted one bit for bit.  A reference (mmcv) checkpoint has no meta['runner']: it resumes too, with a warning
        that the augmentation streams start over.  -> the epoch the run continues with (0-based)."""
        from . import ops
        if path == "auto":
            path = os.path.join(self.work_dir, "latest.pth")
            if not os.path.exists(path):
                return None
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        self.trainer.load_checkpoint(ckpt)
        meta = ckpt.get("meta") or {}
        state = meta.get("runner")
        if state is None:
            warnings.warn(f"{path} has no meta['runner'] (a reference checkpoint?): weights, optimizer state and counters are "
                          f"resumed, the augmentation and dropout streams restart from their seeds")
        else:
            mine = state["loader"][self.rank] if self.rank < len(state["loader"]) else None
            if mine is not None and hasattr(self.train_loader, "load_state"):
                self.train_loader.load_state(mine)
            ops.DROPOUT_SEED[:] = list(state["dropout_seed"])
            self.best = state.get("best")
            k = int(state.get("cumulative_iters", 1))
            if k != self.cumulative_iters:
                warnings.warn(f"{path} was written with cumulative_iters={k}, this run uses {self.cumulative_iters}: accepted, "
                              f"accumulation windows never cross an epoch boundary and checkpoints are written at epoch ends "
                              f"(the effective batch, and with it the suitable rate, changes)")
        self.epoch = int(meta.get("epoch", 0) or 0)
        return self.epoch
