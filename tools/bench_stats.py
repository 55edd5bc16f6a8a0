#!/usr/bin/env python3
"""
Time the threshold sweep of K candidate networks over a resident validation set: ``TrainerGroup.stats`` (forward pass and
counting on the device, integers and two doubles back) against ``evaluate_models(want_probs=True)`` -- the same forward pass,
K x N probabilities back -- followed by the counting on the host, (a) as the reference writes it, a broadcast compare into an
N x T boolean array per network (annoyance_estimator.py:83-84), and (b) as numpy does it best, ``np.searchsorted`` into the
sorted table plus ``np.bincount``.  All three produce the four counts per (network, threshold); they are checked for equality.

    python tools/bench_stats.py [--samples 50000] [--thresholds 1000] [--out profiles/stats/bench_stats.json]

7 timed repetitions after 3 warm-up calls; median and min - max in milliseconds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from mycroft_precise_amd import simulate                       # noqa: E402
from mycroft_precise_amd.model import ModelParams              # noqa: E402
from mycroft_precise_amd.train import TrainerGroup             # noqa: E402

WARMUP, REPS = 3, 7


def timed(fn):
    for _ in range(WARMUP):
        out = fn()
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, {'median_ms': float(np.median(ms)), 'min_ms': min(ms), 'max_ms': max(ms)}


def host_broadcast(probs, y, thr):
    pos, neg = y > 0.5, y == 0
    out = []
    for p in probs:
        wide = p.astype(np.float64).reshape(-1, 1)
        gt, ge = wide > thr.reshape(1, -1), wide >= thr.reshape(1, -1)
        out.append([gt[pos].sum(axis=0), gt[neg].sum(axis=0), ge[pos].sum(axis=0), ge[neg].sum(axis=0)])
    return np.array(out)


def host_searchsorted(probs, y, thr):
    pos, neg = y > 0.5, y == 0
    out = []
    for p in probs:
        wide = p.astype(np.float64)
        row = []
        for side in ('left', 'right'):              # thresholds below p / not above p
            bins = np.searchsorted(thr, wide, side=side)
            for cls in (pos, neg):
                hist = np.bincount(bins[cls], minlength=thr.size + 1)
                row.append(hist[::-1].cumsum()[::-1][1:])
        out.append(row)
    return np.array(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--samples', type=int, default=50000)
    ap.add_argument('--thresholds', type=int, default=1000)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'stats', 'bench_stats.json'))
    args = ap.parse_args()

    rng = np.random.default_rng(0)
    x = rng.normal(0.0, 1.0, (args.samples, 29, 13)).astype(np.float32)
    y = (rng.random(args.samples) < 0.3).astype(np.float32)
    thr = simulate.default_thresholds() if args.thresholds == 1000 else np.linspace(0.0, 1.0, args.thresholds)
    results = {'samples': args.samples, 'thresholds': int(thr.size), 'warmup': WARMUP, 'repetitions': REPS, 'compare': 'f64', 'cases': []}
    for K in (1, 4, 16):
        group = TrainerGroup([ModelParams(recurrent_units=20)] * K, seeds=list(range(K)), n_features=29)
        group._t.set_validation(x, y)
        sweeps, device = timed(lambda: group.stats(thr, compare='f64'))
        probs, forward = timed(lambda: group._t.evaluate_models(source='validation', want_probs=True)[2])
        a, broadcast = timed(lambda: host_broadcast(probs, y, thr))
        b, searchsorted = timed(lambda: host_searchsorted(probs, y, thr))
        got = np.array([[s.counts[f] for f in ('pos_gt', 'neg_gt', 'pos_ge', 'neg_ge')] for s in sweeps])
        assert np.array_equal(got, a) and np.array_equal(got, b), 'the three ways of counting disagree'
        case = {'n_models': K, 'device_stats': device, 'evaluate_models_want_probs': forward, 'host_broadcast_compare': broadcast,
                'host_searchsorted': searchsorted,
                'evaluate_plus_broadcast_median_ms': forward['median_ms'] + broadcast['median_ms'],
                'evaluate_plus_searchsorted_median_ms': forward['median_ms'] + searchsorted['median_ms']}
        results['cases'].append(case)
        print(json.dumps(case), flush=True)
        group.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(results, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
