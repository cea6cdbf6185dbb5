"""Host restatements the log-window and runner tests compare with: pack (numpy f32, one add at a time), accumulate / flush
(Python floats = f64), the cross-rank merge of a validation and the log schedule.  No GPU, no package code."""
import math
from collections import OrderedDict

import numpy as np

F32 = np.float32


def pack_ref(losses):
    """{name: f32 value | [f32 values]} -> (names + ('loss',), [np.float32]) as EncoderDecoder._parse_losses computes them for
    one-element terms: a plain entry is 0 + v (torch's mean reduces from +0.0, so -0.0 comes out +0.0), a list entry
    0 + v0 + v1 + ..., the total 0 + every entry whose name contains 'loss', in dict order; every add rounded to f32."""
    names, vals = [], []
    with np.errstate(all="ignore"):
        for name, value in losses.items():
            acc = F32(0.0)
            for v in (value if isinstance(value, list) else [value]):
                acc = F32(acc + F32(v))
            names.append(name)
            vals.append(acc)
        total = F32(0.0)
        for name, v in zip(names, vals):
            if "loss" in name:
                total = F32(total + v)
    return tuple(names) + ("loss",), vals + [total]


def bits32(v):
    return int(np.asarray(v, dtype=np.float32).view(np.uint32))


def bits64(v):
    return int(np.asarray(v, dtype=np.float64).view(np.uint64))


class HostWindow:
    """tt_logvars_accumulate / tt_logvars_flush in Python floats: `sums` then [total weight, iterations, skipped]."""

    def __init__(self, n_all):
        self.n_all = n_all
        self.w = [0.0] * (n_all + 3)

    def add(self, values, weight, gate=None):
        """values: the n_all f32 values of one iteration (packed then tail), as Python floats."""
        assert len(values) == self.n_all
        if gate is not None and not math.isfinite(gate):
            self.w[self.n_all + 2] += 1.0
            return
        for i, v in enumerate(values):
            self.w[i] += float(v) * float(weight)
        self.w[self.n_all] += float(weight)
        self.w[self.n_all + 1] += 1.0

    def flush(self):
        out, self.w = self.w, [0.0] * (self.n_all + 3)
        return out


def window_means(names, flushed):
    """What logvars.PendingLog.result() returns for a flushed window."""
    n = len(names)
    total = flushed[n]
    out = OrderedDict((k, flushed[i] / total if total else float("nan")) for i, k in enumerate(names))
    out["num_samples"], out["iterations"], out["skipped"] = int(flushed[n]), int(flushed[n + 1]), int(flushed[n + 2])
    return out


def merge_ref(parts):
    """The reference's merge of per-rank validation results (eval_tool.py:146-160), for parts[r] = {name: (mean, count)} in
    rank order: weighted sums and counts grow rank by rank from 0.0, one division per name at the end."""
    weighted, seen = {}, {}
    for part in parts:
        for name in part:
            if name not in weighted:
                weighted[name] = 0.0
                seen[name] = 0.0
            weighted[name] += part[name][0] * part[name][1]
            seen[name] += part[name][1]
    for name in weighted:
        weighted[name] /= seen[name]
    return weighted


def log_schedule_ref(iters, interval, ignore_last):
    """Inner iterations (1-based) whose end writes a train log line: a window closes every `interval` iterations; what is
    left at the end of the epoch is written only when ignore_last is off."""
    out, filled = [], 0
    for i in range(1, iters + 1):
        filled += 1
        if filled == interval:
            out.append(i)
            filled = 0
    if filled and not ignore_last:
        out.append(iters)
    return out
