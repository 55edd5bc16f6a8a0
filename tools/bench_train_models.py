"""One training step of K networks in one trainer (pe_trainer_step_models) against K steps of K separate trainers.

    python tools/bench_train_models.py [--samples 50000] [--reps 7] [--warmup 3] [--out profiles/train/bench_train_models.json]

Stock shape (29 x 13 features, 20 units), the dataset of tools/bench_train.py (50 000 seeded samples resident on the device),
dropout 0.2, loss_bias 0.7, RMSprop with the Keras defaults.  For K in {1, 2, 4, 8, 16} and batches of 1000 and 5000 random
rows, two things are timed with a host clock around whole calls (each ends in a synchronous read of its losses), after `warmup`
discarded calls; median, minimum and maximum of `reps` repetitions are reported:

  * group:     ONE ``HipTrainer.step_models`` call of a trainer that owns K stock networks (two launches, one dataset);
  * separate:  K consecutive ``HipTrainer.step`` calls on K trainers of one network each, every one with a dataset of its
               own -- the plain loop over trainers, in the same process.

``ratio`` = separate median / group median (above 1: the group is faster); ``beyond_spread`` says whether the group's slowest
repetition still beat the separate trainers' fastest.  The same again for one mixed group of widths 8, 20, 20 and 32.
One JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mycroft_precise_amd import synth                      # noqa: E402
from mycroft_precise_amd._lib import HipTrainer            # noqa: E402

RATE, LOSS_BIAS, LR, RHO, EPS = 0.2, 0.7, 1e-3, 0.9, 1e-7
COUNTS, BATCHES, MIXED = (1, 2, 4, 8, 16), (1000, 5000), (8, 20, 20, 32)


def timed(call, batches, warmup, reps):
    for i in range(warmup):
        call(batches[i % len(batches)], i)
    out = []
    for i in range(reps):
        t0 = time.perf_counter()
        call(batches[(warmup + i) % len(batches)], warmup + i)
        out.append(time.perf_counter() - t0)
    return out


def stats(times):
    return {'median': round(1e3 * float(np.median(times)), 4), 'min': round(1e3 * min(times), 4), 'max': round(1e3 * max(times), 4)}


def compare(widths, separate, x, y, batches, warmup, reps):
    """`separate`: trainers of one network each, widths[m] units wide, the dataset already resident"""
    group = HipTrainer([synth.make_weights(13, (h,)) for h in widths], 29, 13)
    group.set_data(x, y)
    seeds = list(range(1, len(widths) + 1))

    def group_step(idx, step):
        return group.step_models(idx, step=step, dropout_rate=RATE, seed=seeds, loss_bias=LOSS_BIAS, lr=LR, rho=RHO, eps=EPS)

    def separate_steps(idx, step):
        return [t.step(idx, RATE, seed, step, LOSS_BIAS, LR, RHO, EPS, 0) for t, seed in zip(separate, seeds)]

    res = {}
    for batch, idx in batches.items():
        g = timed(group_step, idx, warmup, reps)
        s = timed(separate_steps, idx, warmup, reps)
        res[str(batch)] = {'group_ms': stats(g), 'separate_ms': stats(s),
                           'ratio': round(float(np.median(s)) / float(np.median(g)), 3), 'beyond_spread': bool(max(g) < min(s)),
                           'group_samples_per_s': round(len(widths) * batch / float(np.median(g)), 1)}
    group.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--samples', type=int, default=50000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps must be at least 5 (the median of fewer repetitions is not reported)')
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 1.0, (args.samples, 29, 13)).astype(np.float32)
    y = (rng.random(args.samples) < 0.5).astype(np.float32)
    batches = {b: [rng.choice(args.samples, b, replace=False).astype(np.int32) for _ in range(8)] for b in BATCHES}

    def single(h):
        t = HipTrainer(synth.make_weights(13, (h,)), 29, 13)
        t.set_data(x, y)
        return t

    res = {'samples': args.samples, 'reps': args.reps, 'warmup': args.warmup, 'shape': [29, 13, 20], 'dropout': RATE, 'stock': {}}
    stock = [single(20) for _ in range(max(COUNTS))]
    for k in COUNTS:
        res['stock'][str(k)] = compare((20,) * k, stock[:k], x, y, batches, args.warmup, args.reps)
    for t in stock:
        t.close()
    mixed = [single(h) for h in MIXED]
    res['mixed'] = {'widths': list(MIXED), **compare(MIXED, mixed, x, y, batches, args.warmup, args.reps)}
    for t in mixed:
        t.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
