"""One data-parallel training iteration (reference: mmcv EpochBasedRunner.run_iter -> model.train_step
(encoder_decoder_framework.py:140-145) + OptimizerHook (loss.backward(), grad clip, AdamW.step; configs/thinktwice.py:282-290)
under MMDistributedDataParallel (apis/mmdet_train.py:67-74)).

    forward_train on the HIP forward  ->  reverse sweep of the tape (thinktwice_amd/autodiff.py: hand-written backward kernels,
    gradients under the reference's state_dict names)  ->  ONE launch that gathers them into the flat gradient buffer
    (masters.FlatLayout.deposit: the hand-over the torch-autograd route uses too)  ->  ONE all-reduce of that buffer
    (grad_sync.py, RCCL)  ->  global-norm clip + AdamW on the flat buffers (optim.py, two launches)  ->  operands re-prepared
    from the master weights.

`Trainer.step` is one body: a plain iteration is an accumulation window of one with the unscaled gradient; where the two forms
differ (when the counters move, what reconcile() takes back, the `updated` key) the body asks `plain`.

The master parameters are f32 views of one flat buffer (288 GB of HBM: master weights, Adam moments, the flat gradient and the
kernels' operand formats all stay resident).  BatchNorm runs on its running statistics (frozen-BN fine-tuning, what golden F10 /
F13 pin); its affine parameters train, its statistics are not updated.  Parameters the loss never reaches (the reference's 90
dead ones) keep zero gradients, as under DDP's find_unused_parameters.
"""
import contextlib
import os
import sys

import torch

from . import autodiff, masters, ops
from ._lib import TTError
from .grad_sync import FlatGradBuffer
from .masters import BUFFERS as _BUFFERS, trainable as _trainable  # noqa: F401  (the layout rule, shared with the autograd route)
from .optim import FlatAdamW


class Trainer:
    def __init__(self, model, state_dict, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-7, max_grad_norm=100.0,
                 x3=None, frozen_bn=True):
        """`model`: an EncoderDecoder (dtype torch.float32 or "f32x3"); `state_dict`: reference-format weights.  `x3`: input
        gradients of the convolutions through the bf16x3 kernel (default: when the model's forward uses it).
        `frozen_bn=False`: the reference's training semantics (model.train(): batch-statistics BatchNorm with SyncBN across
        the ranks, running statistics updated in `self.buffers`, live ASPP dropout; goldens F11 / F16).  `frozen_bn=True`:
        BatchNorm on its running statistics (model.eval() arithmetic, goldens F10 / F13) -- fine-tuning with frozen
        statistics; the BatchNorm affine parameters still train."""
        if getattr(model, "trainable", False):
            raise TTError("Trainer: this model was built with trainable=True and owns its master weights (torch autograd "
                          "route); a Trainer keeps its own -- build the model without trainable=True")
        dev = model.device
        self.model = model
        self.frozen_bn = bool(frozen_bn)
        self.x3 = (model.dtype != torch.float32) if x3 is None else x3
        sd = masters.strip(state_dict)
        self.layout, self.flat_param, views = masters.flat_masters(sd, dev)
        self.names = self.layout.names
        # (a master view is a leaf whose .grad FlatGradBuffer points into its buffer)
        self._trainable = {k: v.requires_grad_(True) for k, v in views.items()}
        self.sd = {k: self._trainable.get(k, v) for k, v in sd.items()}
        self.grads = FlatGradBuffer([self.sd[k] for k in self.names])
        self.opt = FlatAdamW(self.flat_param, self.grads.flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                             max_grad_norm=max_grad_norm)
        self.param_grads = None
        self._stepped = set()          # names of the parameters the optimizer has updated at least once (torch: those with state)
        self.iteration, self.epoch, self._bn_steps = 0, 0, 0
        self._skips_accounted = 0      # device-skipped updates already taken out of iteration / _bn_steps (reconcile())
        # gradient accumulation (step(window=(j, k))): the open window as (next j, k), the names its micro-steps reached, the
        # closes issued and the skipped windows' micro-iterations accounted since the last reconcile()
        self._window, self._window_names, self._window_closes, self._skipped_iters_accounted = None, set(), 0, 0
        self._seg_table, self._window_scales, self._issued_seen = None, {}, 0
        self.schedule = None           # set_schedule(): the reference's lr_config
        self._prepare_on_device = os.environ.get("TT_TRAIN_PREPARE", "device") != "host"
        # BatchNorm running statistics: device copies the prepared layers alias (train mode updates them in place)
        self.buffers = {k: v.to(dev, torch.float32).contiguous() for k, v in self.sd.items()
                        if torch.is_tensor(v) and k.endswith(("running_mean", "running_var"))}
        self._dev_buffers = self.buffers
        if not self.frozen_bn and not self._prepare_on_device:
            raise ValueError("Trainer(frozen_bn=False) keeps the running statistics on the device: TT_TRAIN_PREPARE=host "
                             "is a frozen-BN path")
        self._prepare()

    def _prepare(self):
        """(Re)build the kernels' operand formats (folded BatchNorm affines, channel-last / pair-split weights) from the
        master weights.  Device path: the load code runs on views of the flat master buffer (BatchNorm statistics moved to
        the device once), so nothing crosses PCIe.  TT_TRAIN_PREPARE=host takes the route a checkpoint takes instead (one
        0.5 GB device-to-host copy + host-side preparation per iteration); it is also the fallback if the load code meets
        a host-only operation on a device tensor."""
        if self._prepare_on_device:
            try:
                masters.prepare_on_device(self.model, self._operand_tensors(), self.frozen_bn)
                return
            except (RuntimeError, TypeError) as e:
                print(f"[trainer] device-side operand preparation failed ({type(e).__name__}: {e}); "
                      f"using the host path", file=sys.stderr, flush=True)
                self._prepare_on_device = False
        autodiff.clear_metas(self.model)
        with torch.no_grad():
            self.model.load_state_dict({k: (v.detach().cpu() if k in self._trainable else v) for k, v in self.sd.items()})

    def _operand_tensors(self):
        return masters.operand_tensors(self.sd, self._trainable, self._dev_buffers, other=self.sd)

    def _sweep(self, batch, device_log):
        """Forward + losses + reverse sweep under this trainer's BatchNorm mode -> (train_step's dict, the swept tape)."""
        was_training = self.model.training
        self.model.train(not self.frozen_bn)
        try:
            with autodiff.Tape(x3=self.x3, release=True) as tape:
                out = self.model.train_step(batch, None, device_log=True) if device_log else self.model.train_step(batch, None)
                tape.backward()
        finally:
            self.model.train(was_training)
        return out, tape

    def _gradients(self, batch, device_log, scale=None, accumulate=False):
        """Forward + losses + reverse sweep, then the tape's parameter gradients into the flat buffer (masters.FlatLayout.deposit,
        one launch): flat (=|+=) scale * g, `param_grads` = the tape's.  Not accumulating, the buffer is zeroed first and the
        deposit WRITES (never 0 * old + scale * g: a NaN left by a skipped update does not survive)."""
        if not accumulate:
            self.grads.zero_()
        out, tape = self._sweep(batch, device_log)
        if self._seg_table is None:
            # two tables in turn: uploading one waits for ITS previous upload only, two deposits back
            self._seg_table = [ops.GradSegTable(self.flat_param.device) for _ in range(2)]
        self._seg_table.reverse()
        self.layout.deposit(self._seg_table[0], tape.param_grads, self.grads.flat, scale, accumulate)
        self.param_grads = tape.param_grads
        return out

    def backward(self, batch, device_log=False):
        """Forward + losses + reverse sweep: fills the flat gradient buffer with the unscaled gradients and sets `param_grads`
        and `live_ranges` (no collective, no update).  Returns dict(loss, log_vars, num_samples) of train_step (`device_log`:
        its device-resident form)."""
        out = self._gradients(batch, device_log)
        self.live_ranges = self.layout.live_ranges(self.param_grads)
        return out

    def set_schedule(self, total_iters, iters_per_epoch, warmup_iters=1000, warmup_ratio=1.0 / 3, min_lr_ratio=1e-3):
        """The reference's `lr_config` (configs/thinktwice.py:286-291: cosine annealing BY EPOCH with a per-iteration linear
        warm-up, optim.warmup_cosine_lr): from now on step() without an explicit `lr` uses the rate of `self.iteration`, and
        `self.epoch` follows the iteration count (EpochBasedRunner)."""
        if not iters_per_epoch or iters_per_epoch < 1:
            raise ValueError("set_schedule: iters_per_epoch (len(data_loader)) is required for the by-epoch cosine")
        self.schedule = dict(total_iters=int(total_iters), iters_per_epoch=int(iters_per_epoch), warmup_iters=int(warmup_iters),
                             warmup_ratio=float(warmup_ratio), min_lr_ratio=float(min_lr_ratio))

    def current_lr(self):
        if self.schedule is None:
            return self.opt.lr
        from .optim import warmup_cosine_lr
        return warmup_cosine_lr(self.opt.lr, self.iteration, **self.schedule)

    def reconcile(self):
        """Blocking.  With check_finite=False the host runs ahead of the device, which skips the update of an iteration whose
        gradient norm is not finite (p, m, v and the applied-step count untouched; non-finite batch statistics never reach
        the BatchNorm running buffers either, tt_bn_finalize).  This takes those skipped iterations back out of the host's
        counters (`iteration`, the BatchNorm call count) so that checkpoints agree with the device; called by state_dict() /
        optimizer_state_dict() / checkpoint().  Returns the number of skipped updates found.

        Accumulation windows: a skipped update is a skipped WINDOW, and `iteration` goes back by the window's length, which
        the device recorded (tt_adamw_advance_window: remainder windows are shorter than k).  `_bn_steps` does NOT go back for
        a skipped window: its micro-steps' forwards ran, their batch statistics went into the running buffers when they ran,
        and torch's num_batches_tracked counts train-mode forwards, not optimizer updates -- the counter stays with what the
        device holds.  Between two reconciles the steps are either all plain or all window closes (step() reconciles where the
        form changes), so one applied-step count tells both cases apart."""
        k = self.opt.skipped() - self._skips_accounted
        windows, self._window_closes, self._issued_seen = self._window_closes, 0, self.opt.issued
        if windows:
            lost = self.opt.skipped_iters() - self._skipped_iters_accounted
            self._skipped_iters_accounted += lost
            self.iteration -= lost
            self._skips_accounted += max(k, 0)
            if self.schedule is not None:
                self.epoch = self.iteration // self.schedule["iters_per_epoch"]
            return max(k, 0)
        if k > 0:
            self.iteration -= k
            if not self.frozen_bn:
                self._bn_steps -= k
            self._skips_accounted += k
            if self.schedule is not None:
                self.epoch = self.iteration // self.schedule["iters_per_epoch"]
        return max(k, 0)

    # ---- gradient accumulation (mmcv GradientCumulativeOptimizerHook(cumulative_iters=k); the window policy is the caller's:
    # runner.accumulation_plan)
    @property
    def window_open(self):
        """An accumulation window has taken a micro-step and is not closed yet."""
        return self._window is not None

    def abandon_window(self):
        """Drop an open window (after an exception inside one of its micro-steps): the next window=(0, k) starts clean.  The
        counters keep the micro-steps taken."""
        self._window = None

    def _no_open_window(self, what):
        if self._window is not None:
            raise TTError(f"Trainer.{what}: accumulation window open at micro-step {self._window[0]} of {self._window[1]}; a "
                          f"half-summed gradient is not something a checkpoint holds -- close the window first")

    def _count_iteration(self):
        self.iteration += 1
        if not self.frozen_bn:
            self._bn_steps += 1
        if self.schedule is not None:
            self.epoch = self.iteration // self.schedule["iters_per_epoch"]

    def step(self, batch, lr=None, check_finite=True, device_log=False, window=None):
        """One iteration; adds `grad_norm` (device tensor [norm, clip factor]) to train_step's dict.  A non-finite gradient
        norm never reaches the weights: tt_grad_norm_clip hands the update a NaN factor and tt_adamw_step_dev skips (p, m, v
        and the device-side step count untouched).  `check_finite` (one host sync per iteration) additionally raises here;
        pass False to look at `grad_norm` whenever convenient (reconcile() squares the host counters with what the device
        applied).  That alone does not make the step asynchronous: the float `log_vars` are read from the device every
        iteration.  With `device_log=True` as well they stay there (a logvars.DeviceLogVars, for a logvars.LogWindow) and the
        step issues no host synchronisation of its own.  Without `lr`, the rate of set_schedule() (else the constructor's).

        `window=(j, k)`: micro-step j (0-based) of a gradient-accumulation window of k; the dict then also carries `updated`.
        Every micro-step runs forward + reverse sweep and deposits the gradients scaled by 1/k (mmcv: loss / k before
        backward): j == 0 writes, j > 0 adds.  j < k - 1 does nothing else (no collective, no clip, no AdamW, no operand
        preparation, no host synchronisation; `grad_norm` None, `updated` False, `check_finite` has nothing to look at).
        j == k - 1 closes: one all-reduce, clip + AdamW over the union of the micro-steps' live ranges at the closing
        iteration's rate, operands re-prepared; `updated` True.  `window=None`, the plain iteration, is the window (0, 1)
        with the unscaled gradient, except where `plain` is asked below."""
        plain = window is None
        if plain:
            j, k = 0, 1
            if self._window is not None:
                raise ValueError(f"Trainer.step: window=None while an accumulation window is open (next: micro-step "
                                 f"{self._window[0]} of {self._window[1]})")
            if self._window_closes:
                self.reconcile()   # plain steps after window closes: one blocking read where the form changes, none after it
        else:
            j, k = (int(v) for v in window)
            if not (k >= 1 and 0 <= j < k):
                raise ValueError(f"Trainer.step: window=({j}, {k}) is not a micro-step j of k with 0 <= j < k")
            if self._window is None and j != 0:
                raise ValueError(f"Trainer.step: window=({j}, {k}) with no window open; a window starts at micro-step 0")
            if self._window is not None and (j, k) != self._window:
                raise ValueError(f"Trainer.step: window=({j}, {k}) does not continue the open window, whose next micro-step is "
                                 f"{self._window[0]} of {self._window[1]}")
            if j == 0 and self.opt.issued - self._issued_seen > self._window_closes:
                self.reconcile()   # window closes after plain steps: the same single read
            if k not in self._window_scales:
                self._window_scales[k] = torch.full((1,), 1.0 / k, dtype=torch.float32, device=self.flat_param.device)
        closes = j == k - 1
        if closes and lr is None and self.schedule is not None:
            lr = self.current_lr()
        if j == 0:
            self._window_names = set()
        out = self._gradients(batch, device_log, None if plain else self._window_scales[k], accumulate=j > 0)
        self._window = None if closes else (j + 1, k)
        self._window_names.update(self.param_grads)
        if not plain:
            # a window's counters (and the running statistics, the dropout counter) move on every micro-step: a skipped close
            # is taken back by reconcile() through the device's skipped_iters (see there for `_bn_steps`, which stays)
            self._count_iteration()
        if not closes:
            out["grad_norm"], out["updated"] = None, False
            return out
        self.live_ranges = self.layout.live_ranges(self._window_names)
        self.grads.all_reduce_mean()
        out["grad_norm"] = self.opt.step(lr, live_ranges=self.live_ranges, window_len=None if plain else k)
        if not plain:
            out["updated"] = True
            self._window_closes += 1
        if check_finite and not bool(torch.isfinite(out["grad_norm"][0])):
            if plain:
                self._skips_accounted += 1          # nothing below runs: iteration / BatchNorm counters never saw this step
                raise FloatingPointError("Trainer.step: non-finite gradient norm; the update was skipped on the device (weights, "
                                         "Adam moments and running statistics of the optimizer are those of the last good step)")
            self.reconcile()                        # takes the window's k micro-iterations back out of `iteration`
            raise FloatingPointError("Trainer.step: non-finite gradient norm at the close of an accumulation window; the update "
                                     "was skipped on the device (weights, Adam moments and the step count are those of the last "
                                     "good update)")
        self._stepped.update(self._window_names)
        if plain:
            # a plain step counts itself once the update is known to be issued for good; one the device skips unseen
            # (check_finite=False) is taken back by reconcile(), `_bn_steps` included
            self._count_iteration()
        self._prepare()
        return out

    @contextlib.contextmanager
    def evaluating(self):
        """`with trainer.evaluating():` -- the model as `model.eval()` sees it, for a validation pass between steps
        (runner.validate; eval_hooks.py:116-152).  The operands are re-prepared for running-statistics BatchNorm from the
        masters and buffers as they stand (a frozen_bn=False trainer prepares for batch statistics after every step), the model
        is put in eval mode; on exit the training preparation and the mode come back.  Parameters, moments, running statistics
        and the counters are not touched."""
        was_training = self.model.training
        if not self._prepare_on_device:
            self._prepare()
        else:
            masters.prepare_on_device(self.model, self._operand_tensors(), True)
        self.model.eval()
        try:
            yield self.model
        finally:
            self.model.train(was_training)
            self._prepare()

    # ---- checkpoints (mmcv CheckpointHook / torch.save layout: meta + state_dict + optimizer)
    def _num_batches_tracked(self, key, value):
        """nn.BatchNorm's call counter under model.train() (masters.bn_calls_per_iteration) after the applied iterations."""
        if self.frozen_bn or self._bn_steps == 0:
            return value
        return value + self._bn_steps * masters.bn_calls_per_iteration(self.model, key)

    def state_dict(self):
        """Reference-format weights (own copies: the master tensors are views of one flat buffer), BatchNorm running
        statistics and `num_batches_tracked` as they stand now."""
        self._no_open_window("state_dict")
        self.reconcile()
        out = {}
        for k, v in self.sd.items():
            if k in self._trainable:
                out[k] = v.detach().clone()
            elif k in self.buffers:
                out[k] = self.buffers[k].detach().clone().cpu()
            elif k.endswith("num_batches_tracked") and torch.is_tensor(v):
                out[k] = self._num_batches_tracked(k, v.clone())
            else:
                out[k] = v
        return out

    def optimizer_state_dict(self):
        """torch.optim.AdamW.state_dict() layout (what mmcv saves under 'optimizer' and `optimizer.load_state_dict` takes on
        resume, train.py:238 / EpochBasedRunner.resume): per-parameter state keyed by the parameter's index in
        model.parameters() order (= state_dict order without the buffers), plus one param_group.  Parameters that never
        received a gradient carry no state, exactly like torch's `grad is None` ones (the reference's 90 dead parameters)."""
        self._no_open_window("optimizer_state_dict")
        self.reconcile()
        o = self.opt
        steps = o.steps
        state, off = {}, 0
        for idx, k in enumerate(self.names):
            n = self.sd[k].numel()
            if k in self._stepped:
                shape = self.sd[k].shape
                state[idx] = {"step": torch.tensor(float(steps)),
                              "exp_avg": o.m[off:off + n].view(shape).detach().clone().cpu(),
                              "exp_avg_sq": o.v[off:off + n].view(shape).detach().clone().cpu()}
            off += n
        # mmcv's LrUpdaterHook stores the BASE rate under 'initial_lr' and overwrites 'lr' with the scheduled (warmed-up /
        # annealed) one every iteration: write both, so a resume by either side takes the schedule's base from 'initial_lr'
        group = {"lr": self.current_lr(), "initial_lr": o.lr, "betas": tuple(o.betas), "eps": o.eps, "weight_decay": o.wd,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                 "params": list(range(len(self.names)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, osd):
        o = self.opt
        self._skips_accounted = 0                  # (setting the step count restarts the issued / applied bookkeeping)
        self._window_closes = self._skipped_iters_accounted = self._issued_seen = 0
        if "exp_avg" in osd:                       # round-3 flat layout (whole-buffer moments)
            o.load_state_dict(osd)
            self._stepped = set(self.names)
            return
        o.m.zero_()
        o.v.zero_()
        self._stepped = set()
        off, steps = 0, 0
        for idx, k in enumerate(self.names):
            n = self.sd[k].numel()
            st = osd["state"].get(idx, osd["state"].get(str(idx)))
            if st is not None:
                o.m[off:off + n].copy_(st["exp_avg"].reshape(-1).to(o.m.device, torch.float32))
                o.v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1).to(o.v.device, torch.float32))
                steps = max(steps, int(float(st["step"])))
                self._stepped.add(k)
            off += n
        o.steps = steps
        g = (osd.get("param_groups") or [{}])[0]
        # the schedule's BASE rate: mmcv checkpoints carry it as 'initial_lr' ('lr' there is the already scheduled rate of the
        # iteration the checkpoint was written at -- using it as the base would apply the schedule twice)
        o.lr = g.get("initial_lr", g.get("lr", o.lr))
        o.betas = tuple(g.get("betas", o.betas))
        o.eps, o.wd = g.get("eps", o.eps), g.get("weight_decay", o.wd)

    def checkpoint(self, epoch=None):
        """What an mmcv checkpoint holds for a resume (configs/thinktwice.py:292 checkpoint_config, mmcv save_checkpoint):
        `meta` (epoch / iter), `state_dict` (reference key names), `optimizer` (torch AdamW layout)."""
        self._no_open_window("checkpoint")
        self.reconcile()
        return {"meta": {"epoch": self.epoch if epoch is None else epoch, "iter": self.iteration},
                "state_dict": self.state_dict(), "optimizer": self.optimizer_state_dict()}

    def load_checkpoint(self, ckpt):
        self._window = None                        # (a half-summed window does not outlive the weights it was computed on)
        sd = ckpt["state_dict"]
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        with torch.no_grad():
            for k in self.names:
                self.sd[k].copy_(sd[k].to(self.sd[k].device, torch.float32))
            for k, b in self.buffers.items():
                b.copy_(sd[k].to(b.device, torch.float32))
            for k, v in sd.items():
                if k.endswith("num_batches_tracked") and k in self.sd:
                    self.sd[k] = v.clone()
        self._bn_steps = 0
        meta = ckpt.get("meta") or {}
        self.epoch, self.iteration = int(meta.get("epoch", 0) or 0), int(meta.get("iter", 0) or 0)
        if "optimizer" in ckpt:
            self.load_optimizer_state_dict(ckpt["optimizer"])
        else:
            # no optimizer state: rebase the issued / applied step bookkeeping where it stands, so that updates skipped BEFORE
            # this load are not taken out of the freshly loaded iteration count by the next reconcile()
            self.opt.steps = self.opt.steps
            self._skips_accounted = 0
            self._window_closes = self._skipped_iters_accounted = self._issued_seen = 0
        self._prepare()
