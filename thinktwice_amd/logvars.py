"""Logged values that stay on the device: from forward_train's loss terms to the mean of a closed log window, without a host
synchronisation in between (csrc/logvars.hip; the contract of the three entries is in include/thinktwice_hip.h).

    out = trainer.step(batch, check_finite=False, device_log=True)     # out["log_vars"] is a DeviceLogVars
    window.add(out["log_vars"], out["num_samples"], gate=out["grad_norm"], extra={"grad_norm": out["grad_norm"]})
    ...
    pending = window.close()            # queues flush + one device-to-pinned copy + an event; never waits
    if pending.ready():                 # non-blocking
        means = pending.result()        # OrderedDict: window means, then num_samples / iterations / skipped

What it replaces: the `.item()` per logged value of EncoderDecoder._parse_losses (encoder_decoder_framework.py:409-439), the host
accumulation `results[k] += v * batch_size` of custom_multi_gpu_test (eval_tool.py:96-109) and mmcv's LogBuffer.average.  The
arithmetic is theirs: f32 values, weighted f64 sums in call order, one f64 division per name when the window is read.
"""
import ctypes
from collections import OrderedDict

import torch

from . import _lib
from ._lib import check, cur_stream, lib, ptr

MAX_TERMS = _lib.TT_LOGVARS_MAX_TERMS
MAX_NAMES = 64
COUNTERS = ("num_samples", "iterations", "skipped")        # the window's last three doubles


class DeviceLogVars:
    """`log_vars` of a train_step(device_log=True): `names` (the loss dict's keys, then 'loss') and `packed`, one device f32
    per name -- under torch.distributed already averaged over the ranks."""

    def __init__(self, names, packed):
        self.names, self.packed = tuple(names), packed
        if packed.numel() != len(self.names):
            raise ValueError(f"{len(self.names)} names for {packed.numel()} values")

    def to_dict(self):
        """Blocking: the floats `train_step` returns without device_log."""
        return OrderedDict(zip(self.names, self.packed.tolist()))

    def __len__(self):
        return len(self.names)


def torch_packed(losses):
    """(names, packed, loss) by the torch expression of losses.parse_losses: what every term type takes, ~3 launches per
    name.  `loss` is the expression's own sum (it keeps whatever autograd graph the terms carry)."""
    log_vars = OrderedDict()
    for name, value in losses.items():
        if torch.is_tensor(value):
            log_vars[name] = value.mean()
        elif isinstance(value, list):
            log_vars[name] = sum(v.mean() for v in value)
        else:
            raise TypeError(f"{name} is not a tensor or list of tensors")
    loss = sum(v for k, v in log_vars.items() if "loss" in k)
    log_vars["loss"] = loss
    packed = torch.stack([v.detach().to(torch.float32).reshape(()) for v in log_vars.values()])
    return tuple(log_vars), packed, loss


_TABLE = None


def pack(losses):
    """forward_train's dict -> (names, packed, loss), `packed` the n + 1 device floats of parse_losses and `loss` its last
    element (a view).  One-element f32 device terms go through ONE launch of tt_logvars_pack; a term with more elements is
    reduced by its own `.mean()` first (the launch parse_losses issues for it today; the kernel's 0 + v leaves a reduction's
    result as it is) and joins the others.  Anything else -- another dtype, a host tensor, a term that carries an
    autograd graph -- takes `torch_packed`.  More than 64 terms: ValueError.  No host synchronisation either way."""
    global _TABLE
    if "loss" in losses:
        raise ValueError("pack: the loss dict already has a 'loss' entry")
    terms, slots, in_loss = [], [], []
    for s, (name, value) in enumerate(losses.items()):
        if torch.is_tensor(value):
            group = [value]
        elif isinstance(value, list) and value:
            group = value
        elif isinstance(value, list):
            return torch_packed(losses)                      # (sum([]) is the int 0: torch's business)
        else:
            raise TypeError(f"{name} is not a tensor or list of tensors")
        in_loss.append("loss" in name)
        for v in group:
            terms.append(v)
            slots.append(s)
    if len(terms) > MAX_TERMS:
        raise ValueError(f"pack: {len(terms)} loss terms, tt_logvars_pack takes {MAX_TERMS}")
    if not terms or any(not (torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float32 and not v.requires_grad and v.numel() > 0)
                        for v in terms):
        return torch_packed(losses)
    terms = [v if v.numel() == 1 else v.mean() for v in terms]
    dev = terms[0].device
    if any(v.device != dev for v in terms):
        return torch_packed(losses)
    if _TABLE is None:
        _TABLE = _lib.structs()["tt_logvars_terms"]()
    tab, n_slots = _TABLE, len(in_loss)
    for i, (v, s) in enumerate(zip(terms, slots)):
        tab.term[i], tab.slot[i] = v.data_ptr(), s
    for s in range(n_slots):
        tab.in_loss[s] = int(in_loss[s])
    packed = torch.empty(n_slots + 1, dtype=torch.float32, device=dev)
    check(lib().tt_logvars_pack(ctypes.byref(tab), len(terms), n_slots, ptr(packed), cur_stream(dev)), "tt_logvars_pack")
    return tuple(losses) + ("loss",), packed, packed[n_slots]


class PendingLog:
    """A closed window on its way to the host: `ready()` never blocks, `result()` waits for the copy if it has to."""

    def __init__(self, names, host, event, keep):
        self.names, self._host, self._event, self._keep = names, host, event, keep
        self._result = None

    def ready(self):
        return self._result is not None or self._event.query()

    def result(self):
        if self._result is None:
            self._event.synchronize()
            vals = self._host.tolist()
            self._keep = None
            n = len(self.names)
            total = vals[n]
            out = OrderedDict((k, (vals[i] / total if total else float("nan"))) for i, k in enumerate(self.names))
            for k, v in zip(COUNTERS, vals[n:]):
                out[k] = int(v)
            self._result = out
        return self._result


class LogWindow:
    """Weighted f64 sums of DeviceLogVars on the device.  The names are those of the first `add` (plus its `extra` names)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.names = self._log_names = self._extra_names = None
        self.window = None
        self.adds = 0                    # add() calls since the last close(), skipped ones included (host-side count)

    def add(self, log_vars, num_samples, gate=None, extra=None):
        """`gate`: device f32 tensor whose first element decides (not finite: the iteration only counts as skipped) --
        Trainer.step's `grad_norm`.  `extra`: {name: device f32 tensor}, the first element of each is logged too."""
        extra = extra or {}
        if self.names is None:
            if len(log_vars.names) > MAX_NAMES:
                raise ValueError(f"LogWindow: {len(log_vars.names)} names, at most {MAX_NAMES}")
            self._log_names, self._extra_names = tuple(log_vars.names), tuple(extra)
            self.names = self._log_names + self._extra_names
            if len(set(self.names)) != len(self.names):
                raise ValueError(f"LogWindow: duplicate names in {self.names}")
            self.window = torch.zeros(len(self.names) + 3, dtype=torch.float64, device=self.device)
        elif tuple(log_vars.names) != self._log_names or tuple(extra) != self._extra_names:
            raise ValueError(f"LogWindow.add: names {tuple(log_vars.names) + tuple(extra)} differ from the window's {self.names}")
        packed = log_vars.packed
        if not (packed.is_cuda and packed.dtype == torch.float32 and packed.is_contiguous()):
            packed = packed.to(self.device, torch.float32).contiguous()
        tail = None
        if extra:
            for t in extra.values():
                _lib.require_cuda(t)
                assert t.dtype == torch.float32, "LogWindow.add: extra values are device f32 tensors"
            vals = list(extra.values())
            tail = vals[0] if len(vals) == 1 else torch.stack([t.reshape(-1)[0] for t in vals])
        if gate is not None:
            _lib.require_cuda(gate)
            assert gate.dtype == torch.float32, "LogWindow.add: the gate is a device f32 tensor"
        check(lib().tt_logvars_accumulate(ptr(packed), len(self._log_names), ptr(tail), len(self._extra_names), int(num_samples),
                                          ptr(gate), ptr(self.window), cur_stream(self.device)), "tt_logvars_accumulate")
        self.adds += 1

    def close(self):
        """Queue the hand-over of the sums gathered so far and start the next window: flush, one device-to-pinned copy, an
        event.  Never waits."""
        if self.names is None:
            raise ValueError("LogWindow.close: nothing was added")
        n_all = self.window.numel()
        out = torch.empty(n_all, dtype=torch.float64, device=self.device)
        check(lib().tt_logvars_flush(ptr(self.window), n_all, ptr(out), cur_stream(self.device)), "tt_logvars_flush")
        host = torch.empty(n_all, dtype=torch.float64, pin_memory=True)
        host.copy_(out, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(self.device))
        self.adds = 0
        return PendingLog(self.names, host, event, out)
