"""Many clips scored in one call (pe_score_clips) against the per-clip loop it replaces: clips per second.

    python tools/bench_clips.py [--clips 2048] [--reps 7] [--out profiles/clips/bench_clips.json]

2048 seeded clips of 0.5 - 3 s (float32 samples, as load_audio returns them) and the stock model.  Two things are timed,
alternately in the same process, after a warm-up of each, with a host clock around calls that end in a synchronous copy of
their results; the median of `reps` repetitions is kept:

  * batched: ``engine.score_clips(clips, max_samples)`` -- one front-end launch and one network launch per pass;
  * loop:    ``engine.predict(np.stack([vectorize(c) for c in clips]))`` -- the path that exists without the batched call
             (vectorization.vectorize: one copy in, one launch, one copy out per clip; then one predict).

The two results are compared bit for bit before anything is timed.  Also reported: the two launch times of the batched call
from pe_set_timing (HIP events around the front-end launch and the network launch of the last pass), and where the front-end
launch lands against the bytes it has to move (float32 samples in, 64-byte rows out) at the HBM peak of
profiles/measured_peaks.json.  One JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mycroft_precise_amd import synth                      # noqa: E402
from mycroft_precise_amd import vectorization as V         # noqa: E402
from mycroft_precise_amd._lib import HipEngine             # noqa: E402
from mycroft_precise_amd.params import pr                  # noqa: E402


def make_clips(n, seed=7):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(pr.sample_rate // 2, 3 * pr.sample_rate + 1, n)
    longest = int(lengths.max())
    base = [synth.stream_pcm(s, longest).astype(np.float32) / np.float32(32768.0) for s in range(16)]
    return [np.ascontiguousarray(base[i % 16][int(rng.integers(0, longest - int(m) + 1)):][:int(m)]) for i, m in enumerate(lengths)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--clips', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps must be at least 5 (the median of fewer repetitions is not reported)')
    clips = make_clips(args.clips)
    eng = HipEngine(pr, synth.make_weights(), n_streams=1)

    def batched():
        return eng.score_clips(clips, pr.max_samples)

    def loop():
        return eng.predict(np.stack([V.vectorize(c) for c in clips]))

    got, want = batched(), loop()                           # warm-up of both, and the check that they compute the same thing
    if not np.array_equal(got, want):
        raise SystemExit('score_clips and the per-clip loop disagree (max |diff| %g)' % float(np.abs(got - want).max()))
    batched(); loop()
    tb, tl = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter(); batched(); tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); loop(); tl.append(time.perf_counter() - t0)
    eng.set_timing(True)
    ev = [(batched(), eng.last_timing())[1] for _ in range(args.reps)]
    eng.set_timing(False)
    mfcc_ms, gru_ms = float(np.median([e[0] for e in ev])), float(np.median([e[1] for e in ev]))
    b, l = float(np.median(tb)), float(np.median(tl))
    samples = int(sum(len(c) for c in clips))
    kept = int(sum(min(len(c), pr.max_samples) for c in clips))
    moved = 4 * kept + args.clips * pr.n_features * 64       # bytes the front-end launch has to read and write
    res = {'clips': args.clips, 'seconds_of_audio': round(samples / pr.sample_rate, 1), 'reps': args.reps,
           'batched_s': round(b, 6), 'loop_s': round(l, 6),
           'batched_clips_per_s': round(args.clips / b, 1), 'loop_clips_per_s': round(args.clips / l, 1), 'ratio': round(l / b, 2),
           'batched_s_all': [round(x, 6) for x in tb], 'loop_s_all': [round(x, 6) for x in tl],
           'front_end_launch_ms': round(mfcc_ms, 4), 'network_launch_ms': round(gru_ms, 4),
           'front_end_bytes': moved, 'front_end_GBps': round(moved / (mfcc_ms * 1e-3) / 1e9, 1) if mfcc_ms > 0 else None}
    peaks = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'measured_peaks.json')
    try:
        hbm = json.load(open(peaks)).get('hbm_read_gbs')
    except (OSError, ValueError):
        hbm = None
    if hbm and res['front_end_GBps']:
        res['front_end_share_of_hbm_peak'] = round(res['front_end_GBps'] / float(hbm), 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    eng.close()


if __name__ == '__main__':
    main()
