"""Float64 / integer numpy restatements of csrc/eval_metrics.hip (the contract: include/thinktwice_hip.h) and of
evaluate.summarize's arithmetic, written from the contract alone.  Sums are SEQUENTIAL in the stated order
(`np.cumsum(...)[-1]`, not np.sum's pairwise order); the label conventions are checked against oracle/train_ref.py in
tests/test_eval_ref.py."""
from collections import OrderedDict

import numpy as np

STAGE_TERMS = ("wp_ade", "wp_fde", "wp_long", "wp_lat", "mu_l1_0", "mu_l1_1", "sigma_l1_0", "sigma_l1_1")


def seq_sum(values, start=0.0):
    """start + v0 + v1 + ... in that order, f64."""
    v = np.concatenate([[np.float64(start)], np.asarray(values, np.float64).reshape(-1)])
    return float(np.cumsum(v)[-1])


def argmax_lowest(rows):
    """(..., C) -> (argmax with ties to the lowest index, any-NaN flag).  np.argmax returns the first maximum; rows with a NaN
    are flagged and their argmax is meaningless."""
    nan = np.isnan(rows).any(-1)
    safe = np.where(np.isnan(rows), -np.inf, rows)
    return np.argmax(safe, -1), nan


def seg_cell_labels(labels, factor):
    """labels (BN, H, W) -> (BN, H/f, W/f): the pixel (y*f, x*f) of every cell."""
    BN, H, W = labels.shape
    return labels[:, 0:(H // factor) * factor:factor, 0:(W // factor) * factor:factor]


def seg_confusion(logits_cl, labels, num_classes, factor):
    """-> (conf int64 (C, C), bad_label, nonfinite)."""
    C = num_classes
    lab_f = seg_cell_labels(np.asarray(labels, np.float32), factor)
    assert lab_f.shape == logits_cl.shape[:3]
    ok_num = np.isfinite(lab_f) & (np.abs(lab_f) < 1e9)
    lab = np.where(ok_num, np.trunc(np.where(ok_num, lab_f, 0)), -1).astype(np.int64)
    pred, nan = argmax_lowest(np.asarray(logits_cl, np.float32)[..., :C])
    conf = np.zeros((C, C), np.int64)
    bad = nonfinite = 0
    for l, p, n in zip(lab.reshape(-1), pred.reshape(-1), nan.reshape(-1)):
        if l == 255:
            continue
        if l < 0 or l >= C:
            bad += 1
        elif n:
            nonfinite += 1
        else:
            conf[l, p] += 1
    return conf, bad, nonfinite


def depth_cell_bins(gt_depth, factor, d_lo, d_step, D):
    """gt_depth (BN, H, W) f32 -> int (BN, H/f, W/f): 0 = background, k = depth channel k - 1.  f32 arithmetic as stated."""
    g = np.asarray(gt_depth, np.float32)
    BN, H, W = g.shape
    h, w = H // factor, W // factor
    g = g.reshape(BN, h, factor, w, factor).transpose(0, 1, 3, 2, 4).reshape(BN, h, w, factor * factor)
    g = np.where(g == 0, np.float32(1e5), g).min(-1)
    d_lo, d_step = np.float32(d_lo), np.float32(d_step)
    g = ((g - (d_lo - d_step)) / d_step).astype(np.float32)
    g = np.where((g < np.float32(D + 1)) & (g >= 0), g, np.float32(0))
    return np.trunc(g).astype(np.int64)


def depth_bins(logits_cl, gt_depth, D, factor, d_lo, d_step):
    """-> [n_fg, n_top1, n_within1, sum_abs_bins, nonfinite]."""
    bins = depth_cell_bins(gt_depth, factor, d_lo, d_step, D)
    pred, nan = argmax_lowest(np.asarray(logits_cl, np.float32)[..., :D])
    fg = bins >= 1
    bad = fg & nan
    use = fg & ~nan
    off = np.abs(pred - (bins - 1))[use]
    return [int(use.sum()), int((off == 0).sum()), int((off <= 1).sum()), int(off.sum()), int(bad.sum())]


def decoder(pred_wp, mu, sigma, pred_speed, wp, a_mu, a_sigma, speed, sums=None, counts=None):
    """One call of tt_eval_decoder -> (sums (8 S + 1) f64, [samples, nonfinite]); `sums` / `counts`: the accumulators so far."""
    pred_wp, mu, sigma = (np.asarray(x, np.float32) for x in (pred_wp, mu, sigma))
    pred_speed = np.asarray(pred_speed, np.float32).reshape(-1)
    B, S = pred_wp.shape[:2]
    sums = np.zeros(8 * S + 1) if sums is None else np.array(sums, np.float64)
    counts = [0, 0] if counts is None else list(counts)
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)                                       # noqa: E731
    for b in range(B):
        if not (np.isfinite(pred_wp[b]).all() and np.isfinite(mu[b]).all() and np.isfinite(sigma[b]).all()
                and np.isfinite(pred_speed[b])):
            counts[1] += 1
            continue
        counts[0] += 1
        for s in range(S):
            d = f64(pred_wp[b, s]) - f64(wp[b])                              # (4, 2)
            dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            terms = [seq_sum(dist) * 0.25, dist[3], seq_sum(np.abs(d[:, 0])) * 0.25, seq_sum(np.abs(d[:, 1])) * 0.25,
                     abs(f64(mu[b, s, 0]) - f64(a_mu[b][0])), abs(f64(mu[b, s, 1]) - f64(a_mu[b][1])),
                     abs(f64(sigma[b, s, 0]) - f64(a_sigma[b][0])), abs(f64(sigma[b, s, 1]) - f64(a_sigma[b][1]))]
            for j, v in enumerate(terms):
                sums[8 * s + j] = sums[8 * s + j] + np.float64(v)
        sums[8 * S] = sums[8 * S] + abs(12.0 * f64(pred_speed[b]) - f64(np.asarray(speed).reshape(-1)[b]))
    return sums, counts


def pair_deviation(a, b):
    """-> (max |a - b| f32, max |a| f32, non-finite elements); the maxima over the elements where both are finite, 0 if none."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    ok = np.isfinite(a) & np.isfinite(b)
    with np.errstate(over="ignore"):
        d = np.abs(a[ok] - b[ok]).astype(np.float32)
    return (np.float32(d.max()) if d.size else np.float32(0), np.float32(np.abs(a[ok]).max()) if d.size else np.float32(0),
            int((~ok).sum()))


def pair_wp(a, b, max_sum=(0.0, 0.0), counts=(0, 0)):
    """-> ([max, sequential sum] of the f64 point distances, [finite points, others])."""
    a, b = np.asarray(a, np.float32).reshape(-1, 2), np.asarray(b, np.float32).reshape(-1, 2)
    ok = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
    d = a[ok].astype(np.float64) - b[ok].astype(np.float64)
    dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return ([max(float(max_sum[0]), float(dist.max()) if dist.size else 0.0), seq_sum(dist, max_sum[1])],
            [counts[0] + int(ok.sum()), counts[1] + int((~ok).sum())])


def pair_seg(a_cl, b_cl, num_classes):
    """-> [cells whose argmax differs, cells compared, cells with a NaN in either]."""
    pa, na = argmax_lowest(np.asarray(a_cl, np.float32)[..., :num_classes])
    pb, nb = argmax_lowest(np.asarray(b_cl, np.float32)[..., :num_classes])
    bad = na | nb
    return [int(((pa != pb) & ~bad).sum()), int((~bad).sum()), int(bad.sum())]


def _div(a, b):
    return a / b if b else float("nan")


def summarize(raw, class_names, d_step):
    """evaluate.summarize restated: raw accumulators -> metrics."""
    out = OrderedDict()
    n = raw["num_samples"]
    sums = list(raw["dec_sums"])
    S = (len(sums) - 1) // 8
    for s in range(S):
        for j, name in enumerate(STAGE_TERMS):
            out[f"{name}_{s}"] = _div(sums[8 * s + j], n)
    out["speed_mae"] = _div(sums[8 * S], n)
    conf = np.asarray(raw["seg_conf"], np.int64)
    tp = np.diag(conf)
    union = conf.sum(0) + conf.sum(1) - tp
    iou = OrderedDict((class_names[c], (int(tp[c]) / int(union[c]) if union[c] else None)) for c in range(len(tp)))
    have = [v for v in iou.values() if v is not None]
    out["seg_iou"] = iou
    out["seg_miou"] = sum(have) / len(have) if have else float("nan")
    out["seg_pixel_acc"] = _div(int(tp.sum()), int(conf.sum()))
    out["seg_bad_label"], out["seg_nonfinite"] = raw["seg_bad_label"], raw["seg_nonfinite"]
    n_fg, n_top1, n_w1, s_abs, d_nf = raw["depth"]
    out["depth_top1"], out["depth_within1"] = _div(n_top1, n_fg), _div(n_w1, n_fg)
    out["depth_mae_m"] = _div(s_abs * d_step, n_fg)
    out["depth_n_fg"], out["depth_nonfinite"] = n_fg, d_nf
    out["nonfinite"] = raw["dec_nonfinite"]
    out["num_samples"] = n
    return out
