"""Noise augmentation (augment.NoiseAugmenter: load + append_to) against the per-copy loop a user writes without it.

    python tools/bench_augment.py [--clips 2000] [--seconds 1.5] [--inflation 5] [--repeats 5] [--seed 1] [--out FILE]

Synthetic audio (synth.stream_pcm as load_audio returns it: k / 32767 in float32): `clips` clips of `seconds` seconds and four
noise recordings of ten seconds each.  One plan over all clips is drawn on the host with random.Random(seed) (its time is
reported; the loop's cursor and draws are the same work).  Then

  * session:  NoiseAugmenter.load(plan) -- every copy's noise volume -- and NoiseAugmenter.append_to(trainer): mix, int16 round
              trip, front end and rows behind the resident set, on the device;
  * loop:     precise-add-noise as restated in tests/augment_reference.py (builtin sum twice per copy, numpy mixing, the int16
              round trip in memory -- no wav file is written), vectorization.vectorize per reloaded copy, the windows stacked
              and Trainer.append of them.

Both put the same float32 rows and targets behind an empty resident set; that they are equal is checked before anything is
timed.  Each side is warmed up once on the full size and then timed `repeats` times, alternating, with a host clock around
work that ends in a synchronous read from the device; the medians and the spread are reported.  One JSON line; --out also
writes it to a file.  The kernels' own times are not in here: take them from a kernel trace of this command.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import augment_reference as ref                                         # noqa: E402
from mycroft_precise_amd import synth, vectorization                    # noqa: E402
from mycroft_precise_amd.augment import NoiseAugmenter                  # noqa: E402
from mycroft_precise_amd.model import ModelParams                       # noqa: E402
from mycroft_precise_amd.network_runner import HipRunner                # noqa: E402
from mycroft_precise_amd.params import pr                               # noqa: E402
from mycroft_precise_amd.train import Trainer                           # noqa: E402


def audio(seed, n):
    return synth.stream_pcm(seed, int(n)).astype(np.float32) / np.float32(32767.0)


def run_session(aug, plan, weights):
    trainer = Trainer(weights, ModelParams(recurrent_units=20))
    t0 = time.perf_counter()
    aug.load(plan)
    t1 = time.perf_counter()
    aug.append_to(trainer)
    last = trainer._t.get_data(first=trainer.n_samples() - 1, n=1)      # a read from the device: everything before it is done
    t2 = time.perf_counter()
    return t2 - t0, t1 - t0, trainer, last


def run_loop(clips, noises, labels, args, weights):
    trainer = Trainer(weights, ModelParams(recurrent_units=20))
    t0 = time.perf_counter()
    copies = ref.run(clips, ref.Pool(noises), random.Random(args.seed), args.inflation)
    rows = [vectorization.vectorize(ref.loaded(ref.saved(c.mix))).astype(np.float32) for c in copies]
    trainer.append(np.stack(rows), labels[[c.clip for c in copies]])
    last = trainer._t.get_data(first=trainer.n_samples() - 1, n=1)
    return time.perf_counter() - t0, trainer, last


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--clips', type=int, default=2000)
    ap.add_argument('--seconds', type=float, default=1.5)
    ap.add_argument('--inflation', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    weights = synth.make_weights(pr.n_mfcc, (20,), seed=7)

    n = int(args.seconds * pr.sample_rate)
    clips = [audio(s, n) for s in range(args.clips)]
    noises = [audio(100000 + s, 10 * pr.sample_rate) for s in range(4)]
    labels = (np.arange(args.clips) % 2).astype(np.float32)
    aug = NoiseAugmenter(HipRunner(weights=weights), clips, noises, labels)
    t0 = time.perf_counter()
    plan = aug.plan(random.Random(args.seed), args.inflation)
    plan_s = time.perf_counter() - t0
    if plan.n_copies == 0:
        raise SystemExit('the plan holds no copy: nothing to time')

    # warm-up at the full size, and the check: the same rows and targets on both sides, no copy out of range
    _, _, ta, _ = run_session(aug, plan, weights)
    _, tb, _ = run_loop(clips, noises, labels, args, weights)
    xa, ya = ta._t.get_data()
    xb, yb = tb._t.get_data()
    rows_equal = xa.tobytes() == xb.tobytes() and ya.tobytes() == yb.tobytes()
    overflowed = int(aug.volumes()[2].sum())
    ta.close(); tb.close()

    session, load, loop = [], [], []
    for _ in range(args.repeats):
        s, l, t, _ = run_session(aug, plan, weights)
        t.close()
        session.append(s); load.append(l)
        s, t, _ = run_loop(clips, noises, labels, args, weights)
        t.close()
        loop.append(s)
    copies, mixed_samples = plan.n_copies, plan.n_copies * n
    ms, ml = float(np.median(session)), float(np.median(loop))
    res = {'clips': args.clips, 'seconds': args.seconds, 'inflation': args.inflation, 'seed': args.seed, 'repeats': args.repeats,
           'copies': copies, 'pieces': int(plan.pieces.size), 'mixed_samples': mixed_samples, 'plan_s': round(plan_s, 4),
           'session_s': round(ms, 5), 'session_min_max_s': [round(min(session), 5), round(max(session), 5)],
           'load_s': round(float(np.median(load)), 5), 'load_min_max_s': [round(min(load), 5), round(max(load), 5)],
           'loop_s': round(ml, 4), 'loop_min_max_s': [round(min(loop), 4), round(max(loop), 4)],
           'session_copies_per_s': round(copies / ms, 1), 'loop_copies_per_s': round(copies / ml, 1), 'loop_over_session': round(ml / ms, 2),
           'overflowed_samples': overflowed, 'rows_equal': bool(rows_equal)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    aug.close()
    if not rows_equal:
        raise SystemExit('the two sides disagree')


if __name__ == '__main__':
    main()
