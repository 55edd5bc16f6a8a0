"""Plain-numpy restatement of what the statistics calls compute (pe_stats_scores and its kin), written for
clarity: the oracle of tests/test_stats.py, itself held to what the reference's own code computed
(tests/golden/stats.npz) by tests/test_stats_host.py."""
import math

import numpy as np


def classes(targets):
    """-> (positive, negative, other) masks: y > 0.5, y == 0, the rest"""
    y = np.asarray(targets, dtype=np.float32).reshape(-1)
    pos, neg = y > 0.5, y == 0
    return pos, neg, ~(pos | neg)


def counts(outputs, targets, thresholds, compare):
    """-> dict of int64 [T] arrays pos_gt, neg_gt, pos_ge, neg_ge.  'f32': the threshold rounded to float32 meets the float32
    prediction (numpy: float32 array against a Python float); 'f64': the prediction widened meets the float64 threshold."""
    p = np.asarray(outputs, dtype=np.float32).reshape(-1)
    pos, neg, _ = classes(targets)
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1, 1)
    if compare == 'f32':
        lhs, thr = p[np.newaxis, :], thr.astype(np.float32)
    else:
        lhs = p.astype(np.float64)[np.newaxis, :]
    gt, ge = lhs > thr, lhs >= thr                    # [T, n]; a NaN prediction is above nothing
    return {'pos_gt': (gt & pos).sum(axis=1, dtype=np.int64), 'neg_gt': (gt & neg).sum(axis=1, dtype=np.int64),
            'pos_ge': (ge & pos).sum(axis=1, dtype=np.int64), 'neg_ge': (ge & neg).sum(axis=1, dtype=np.int64)}


def fit_logits(outputs, targets):
    """x = -log(u) in float64 with u = float32(float32(1 / p) - 1), over the unsaturated predictions on positive targets"""
    p = np.asarray(outputs, dtype=np.float32).reshape(-1)
    pos, _, _ = classes(targets)
    fit = pos & ~np.isnan(p) & (p != 0) & (p != 1)
    with np.errstate(divide='ignore'):
        u = np.float32(1) / p[fit] - np.float32(1)
        assert u.dtype == np.float32
        return -np.log(u.astype(np.float64))


def summary(outputs, targets):
    """-> dict: the integer fields of pe_stats_summary and logit_mean / logit_std with exactly rounded sums (math.fsum)"""
    p = np.asarray(outputs, dtype=np.float32).reshape(-1)
    pos, neg, other = classes(targets)
    unsaturated = ~np.isnan(p) & (p != 0) & (p != 1)
    x = fit_logits(p, targets)
    n_fit = len(x)
    mean = math.fsum(x) / n_fit if n_fit else float('nan')
    std = math.sqrt(math.fsum((x - mean) ** 2) / n_fit) if n_fit else float('nan')
    return {'n': p.size, 'n_pos': int(pos.sum()), 'n_neg': int(neg.sum()), 'n_other': int(other.sum()), 'n_nan': int(np.isnan(p).sum()),
            'n_unsaturated': int(unsaturated.sum()), 'n_fit': n_fit, 'logit_mean': mean, 'logit_std': std}


def literal_mu_std(outputs, targets):
    """calc_threshold.py:66-77 as numpy evaluates it on float32 predictions (float32 logarithm, numpy's mean), without the
    smoothing factor: what the float64 contract is NOT, kept to record the distance"""
    p = np.asarray(outputs, dtype=np.float32).reshape(-1)
    y = np.asarray(targets, dtype=np.float32).reshape(-1)
    keep = (p != 0) & (p != 1)
    inv = -np.log(1 / p[keep] - 1)
    chosen = inv[y[keep] > 0.5]
    mu = chosen.mean().item()
    return mu, math.sqrt(np.mean((chosen - mu) ** 2))


def confusion(outputs, targets, threshold):
    """Stats.to_dict / num_correct at one threshold for 0 / 1 targets, from the counts above (compare 'f32')"""
    c = counts(outputs, targets, [threshold], 'f32')
    pos, neg, other = classes(targets)
    assert not other.any()
    n_pos, n_neg = int(pos.sum()), int(neg.sum())
    return {'true_pos': int(c['pos_gt'][0]), 'false_pos': int(c['neg_gt'][0]), 'false_neg': n_pos - int(c['pos_gt'][0]),
            'true_neg': n_neg - int(c['neg_gt'][0]), 'num_correct': int(c['pos_ge'][0]) + n_neg - int(c['neg_ge'][0])}


def annoyance_thresholds():
    return 1 / (1 + np.exp(-np.linspace(-20, 20, 1000)))


def buckets(predictions, thresholds):
    """predictions above each threshold, the float32 predictions widened (annoyance_estimator.py:70-71, 83-84)"""
    p = np.asarray(predictions, dtype=np.float32).reshape(-1).astype(np.float64)
    return np.array([(p > t).sum() for t in thresholds], dtype=np.int64)


def estimate(ww_predictions, noise_predictions, noise_seconds, interaction_estimate=100, ambient_annoyance=1.0):
    """AnnoyanceEstimator.estimate from predictions: ``ww_predictions`` of the positive samples, ``noise_predictions`` one array
    per noise file, ``noise_seconds`` the files' total length.  -> (annoyance, ww_annoyance, nww_annoyance, threshold,
    ww_annoyances [1000])"""
    thr = annoyance_thresholds()
    n_ww = np.asarray(ww_predictions).size
    miss = 1 - buckets(ww_predictions, thr) / n_ww
    ww = np.full(len(thr), np.inf)
    ok = miss < 0.5
    ww[ok] = 1 / (1 - 2 * miss[ok]) - 1
    ww = interaction_estimate * ww
    total = np.zeros(len(thr))
    for p in noise_predictions:
        total += buckets(p, thr)
    nww = ambient_annoyance * (total * 60 * 60 / noise_seconds) * 24
    both = ww + nww
    k = int(np.argmin(both))
    return both[k], ww[k], nww[k], thr[k], ww
