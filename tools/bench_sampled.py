"""One cycle of sampled training (train.SampledTrainer) against the host loop it replaces.

    python tools/bench_sampled.py [--rows 100000] [--chunk 50] [--cycles 5] [--reps 5] [--epochs 1] [--batch 5000] [--out FILE]

N seeded stock-shape rows (29 x 13) with random targets and a random 20-unit network, so that about half the rows fail and
every cycle finds `chunk` new ones.  Both sides run the cycle of scripts/train_sampled.py:75-90 from the same initial state,
for both orders:

  * resident:  SampledTrainer.cycle -- one sample_choose (forward over the resident set, the choice on the device, a report
               and at most `chunk` ids back) and fit_resident(subset=selected); the set was uploaded once, outside the clock;
  * loop:      trainer.predict(inputs) from host memory, the same choice in numpy (a boolean mask instead of the script's
               per-row md5, which would only slow this side down), trainer.fit(inputs[sel], outputs[sel]).

A repetition is `cycles` consecutive cycles after one warm-up cycle; the figure is seconds per cycle, the median over `reps`
repetitions with the minimum and maximum next to it (a host clock: every cycle of both sides ends in a synchronous read).  One
JSON line per order, with whether both sides selected the same rows and ended with the same weights; --out appends them to
a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mycroft_precise_amd import synth                                   # noqa: E402
from mycroft_precise_amd.model import ModelParams                       # noqa: E402
from mycroft_precise_amd.params import pr                               # noqa: E402
from mycroft_precise_amd.train import SampledTrainer, Trainer           # noqa: E402

SEED = 5


def host_cycle(trainer, x, y, selected, taken, chunk, order, epochs, batch):
    p = trainer.predict(x).reshape(-1)
    cand = np.flatnonzero(((p > 0.5) != (y > 0.5)) & ~taken)
    if order == 'error':
        cand = cand[np.lexsort((cand, -np.abs(p[cand] - y[cand])))]
    new = cand[:chunk]
    taken[new] = True
    selected += new.tolist()
    if selected:
        trainer.fit(x[selected], y[selected], batch_size=batch, epochs=epochs)


def measure(weights, x, y, order, args):
    def trainer():
        return Trainer(weights, ModelParams(recurrent_units=20), seed=SEED)
    names = ['%08x' % i for i in range(len(x))]      # rows of a seeded normal draw are distinct: no md5 of 100 000 rows
    times = {'resident': [], 'loop': []}
    same_rows = same_weights = True
    for _ in range(args.reps):
        a, b = trainer(), trainer()
        st = SampledTrainer(a, x, y, num_sample_chunk=args.chunk, order=order, hashes=names)
        selected, taken = [], np.zeros(len(x), dtype=bool)
        st.cycle(args.epochs, args.batch)                               # warm-up cycle of both sides
        host_cycle(b, x, y, selected, taken, args.chunk, order, args.epochs, args.batch)
        t0 = time.perf_counter()
        for _ in range(args.cycles):
            st.cycle(args.epochs, args.batch)
        t1 = time.perf_counter()
        for _ in range(args.cycles):
            host_cycle(b, x, y, selected, taken, args.chunk, order, args.epochs, args.batch)
        t2 = time.perf_counter()
        times['resident'].append((t1 - t0) / args.cycles)
        times['loop'].append((t2 - t1) / args.cycles)
        same_rows = same_rows and st.selected == selected
        same_weights = same_weights and a._t.get_weights().tobytes() == b._t.get_weights().tobytes()
        a.close()
        b.close()
    res = {'order': order, 'rows': len(x), 'chunk': args.chunk, 'cycles': args.cycles, 'reps': args.reps, 'epochs': args.epochs}
    for side, t in times.items():
        res[side + '_ms'] = {'median': round(1e3 * float(np.median(t)), 3), 'min': round(1e3 * min(t), 3), 'max': round(1e3 * max(t), 3)}
    res['loop_over_resident'] = round(float(np.median(times['loop']) / np.median(times['resident'])), 2)
    res['same_rows'], res['same_weights'] = bool(same_rows), bool(same_weights)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rows', type=int, default=100000)
    ap.add_argument('--chunk', type=int, default=50)
    ap.add_argument('--cycles', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--epochs', type=int, default=1)
    ap.add_argument('--batch', type=int, default=5000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 1.0, (args.rows, pr.n_features, pr.feature_size)).astype(np.float32)
    y = (rng.random(args.rows) < 0.5).astype(np.float32)
    weights = synth.make_weights(pr.feature_size, (20,), seed=7)
    for order in ('index', 'error'):
        line = json.dumps(measure(weights, x, y, order, args))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
