"""Generated training data (generated.Generator: load + append_to) against the per-chunk loop a user writes without it.

    python tools/bench_generated.py [--minutes 20] [--backgrounds 20] [--chunk 2048] [--repeats 5] [--seed 1] [--out FILE]

Synthetic audio (synth.stream_pcm as load_audio returns it: k / 32767 in float32): `backgrounds` recordings that share
`minutes` of audio, eight wake-word clips of 1.3 .. 1.45 s and eight not-wake-word clips of 0.5 .. 1.2 s.  One plan over all
backgrounds is drawn on the host with random.Random(seed) (its time is reported, it is the same work for both sides).  Then

  * session:  Generator.load(plan) -- mix + every frame once -- and Generator.append_to(trainer, plan.ids, plan.targets);
  * loop:     a float-mode Listener cleared per file, update_vectors per mixed chunk (the chunks are the session's own mixed
              samples, fetched before the clock starts), the emitted windows stacked and Trainer.append of them.

Both put the same float32 rows and targets behind an empty resident set; that they are equal is checked before anything is
timed.  Each side is warmed up once on the full size and then timed `repeats` times, alternating, with a host clock around
work that ends in a synchronous read from the device; the medians and the spread are reported.  One JSON line; --out also
writes it to a file.  The mix kernel's own time is not in here: take it from a kernel trace of this command.
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mycroft_precise_amd import synth                                   # noqa: E402
from mycroft_precise_amd.generated import Generator                     # noqa: E402
from mycroft_precise_amd.model import ModelParams, save_weights         # noqa: E402
from mycroft_precise_amd.network_runner import HipRunner, Listener      # noqa: E402
from mycroft_precise_amd.params import pr                               # noqa: E402
from mycroft_precise_amd.train import Trainer                           # noqa: E402


def audio(seed, n):
    return synth.stream_pcm(seed, int(n)).astype(np.float32) / np.float32(32767.0)


def make_inputs(minutes, n_bg, seed):
    rng = np.random.default_rng(seed)
    total = int(minutes * 60 * pr.sample_rate)
    cuts = np.sort(rng.integers(0, total, n_bg - 1))
    lengths = np.diff(np.concatenate(([0], cuts, [total])))
    backgrounds = [audio(s, n) for s, n in enumerate(lengths)]
    positives = [audio(1000 + s, n) for s, n in enumerate(rng.integers(20800, 23200, 8))]
    negatives = [audio(2000 + s, n) for s, n in enumerate(rng.integers(8000, 19200, 8))]
    return backgrounds, positives, negatives


def run_session(gen, plan, weights):
    trainer = Trainer(weights, ModelParams(recurrent_units=20))
    t0 = time.perf_counter()
    gen.load(plan)
    t1 = time.perf_counter()
    gen.append_to(trainer, plan.ids, plan.targets)
    last = trainer._t.get_data(first=trainer.n_samples() - 1, n=1)      # a read from the device: everything before it is done
    t2 = time.perf_counter()
    return t2 - t0, t1 - t0, trainer, last


def run_loop(lis, mixed, plan, weights, chunk):
    trainer = Trainer(weights, ModelParams(recurrent_units=20))
    emitted = set(plan.ids.tolist())
    t0 = time.perf_counter()
    rows = []
    g = 0
    for samples in mixed:
        lis.clear()
        for a in range(0, len(samples), chunk):
            window = lis.update_vectors(samples[a:a + chunk])
            if g in emitted:
                rows.append(window.astype(np.float32))
            g += 1
    trainer.append(np.stack(rows), plan.targets)
    last = trainer._t.get_data(first=trainer.n_samples() - 1, n=1)
    return time.perf_counter() - t0, trainer, last


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--minutes', type=float, default=20.0)
    ap.add_argument('--backgrounds', type=int, default=20)
    ap.add_argument('--chunk', type=int, default=2048)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    weights = synth.make_weights(pr.n_mfcc, (20,), seed=7)
    model_file = os.path.join(tempfile.mkdtemp(prefix='bench_generated_'), 'random20.npz')
    save_weights(model_file, weights)

    backgrounds, positives, negatives = make_inputs(args.minutes, args.backgrounds, seed=3)
    gen = Generator(HipRunner(weights=weights), backgrounds, positives, negatives, chunk_size=args.chunk)
    t0 = time.perf_counter()
    plan = gen.plan(random.Random(args.seed))
    plan_s = time.perf_counter() - t0
    if plan.ids.size == 0:
        raise SystemExit('the plan holds no sample: nothing to time')
    lis = Listener(model_file, args.chunk)

    # warm-up at the full size, and the check: the same rows and targets on both sides
    _, _, ta, _ = run_session(gen, plan, weights)
    mixed = [gen.audio(f) for f in range(len(plan.files))]
    _, tb, _ = run_loop(lis, mixed, plan, weights, args.chunk)
    xa, ya = ta._t.get_data()
    xb, yb = tb._t.get_data()
    rows_equal = xa.tobytes() == xb.tobytes() and ya.tobytes() == yb.tobytes() == plan.targets.tobytes()
    ta.close(); tb.close()

    session, load, loop = [], [], []
    for _ in range(args.repeats):
        s, l, t, _ = run_session(gen, plan, weights)
        t.close()
        session.append(s); load.append(l)
        s, t, _ = run_loop(lis, mixed, plan, weights, args.chunk)
        t.close()
        loop.append(s)
    n, mixed_samples = int(plan.ids.size), int(plan.n_chunks) * args.chunk
    ms, ml = float(np.median(session)), float(np.median(loop))
    res = {'minutes': args.minutes, 'backgrounds': args.backgrounds, 'chunk': args.chunk, 'seed': args.seed, 'repeats': args.repeats,
           'chunks': int(plan.n_chunks), 'samples': n, 'positives': int(plan.targets.sum()), 'segments': int(plan.segments.size),
           'mixed_samples': mixed_samples, 'mix_bytes': 16 * mixed_samples, 'plan_s': round(plan_s, 4),
           'session_s': round(ms, 5), 'session_min_max_s': [round(min(session), 5), round(max(session), 5)],
           'load_s': round(float(np.median(load)), 5),
           'loop_s': round(ml, 4), 'loop_min_max_s': [round(min(loop), 4), round(max(loop), 4)],
           'session_samples_per_s': round(n / ms, 1), 'loop_samples_per_s': round(n / ml, 1), 'loop_over_session': round(ml / ms, 2),
           'rows_equal': bool(rows_equal)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    gen.close()
    if not rows_equal:
        raise SystemExit('the two sides disagree')


if __name__ == '__main__':
    main()
