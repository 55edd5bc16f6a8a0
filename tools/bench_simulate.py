"""Many long recordings simulated in one call (pe_simulate_clips) against the per-recording loop it replaces.

    python tools/bench_simulate.py [--reps 7] [--workload a|b|both] [--out profiles/simulate/bench_simulate.json]

What precise-simulate and compute_nww_annoyances do per recording (scripts/simulate.py:106-129, annoyance_estimator.py:56-73):
predictions every 4096 samples, a fresh TriggerDetector, two sums, and the windows above each of 1000 thresholds.  Stock
model, float32 samples (as load_audio returns them), two workloads:

  (a) 2048 recordings of 5 - 20 s        (many launches and a long host loop to save)
  (b) 16 recordings of 10 min            (little to save: the audio's way to the device dominates)

Each is run three ways, alternately in the same process, after a check that all three give the same metrics and a warm-up of
each, with a host clock around calls that end in a synchronous copy of their results; the median of `reps` repetitions is kept:

  * simulate:  ``runner.simulate(recordings, thresholds=...)`` -- the metrics computed on the device, no predictions copied back;
  * evaluate:  ``runner.evaluate_clips(recordings)`` plus the host metrics below -- the device part alone is reported as well;
  * loop:      ``runner.evaluate(r)`` per recording, plus for each the Python TriggerDetector, the two numpy sums and the
               ``[n, 1000]`` numpy bucket comparison -- the path that exists without this feature.

Also reported: the front-end and network launch times of the last pass (pe_set_timing), beside which the cost of the metrics
kernels -- simulate against the device part of evaluate, which differ by those kernels and by the predictions' copy back --
can be read.  One JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mycroft_precise_amd import synth                              # noqa: E402
from mycroft_precise_amd.network_runner import HipRunner           # noqa: E402
from mycroft_precise_amd.params import pr                          # noqa: E402
from mycroft_precise_amd.runner import TriggerDetector             # noqa: E402
from mycroft_precise_amd.simulate import default_thresholds        # noqa: E402

CHUNK, THRESHOLD = 4096, 0.5


def base_signals(seconds=20):
    return [synth.stream_pcm(s, seconds * pr.sample_rate).astype(np.float32) / np.float32(32768.0) for s in range(16)]


def workload_a(base, n=2048, seed=11):
    rng = np.random.default_rng(seed)
    longest = len(base[0])
    lengths = rng.integers(5 * pr.sample_rate, longest + 1, n)
    return [np.ascontiguousarray(base[i % 16][int(rng.integers(0, longest - int(m) + 1)):][:int(m)]) for i, m in enumerate(lengths)]


def workload_b(base, n=16, seconds=600):
    reps = seconds * pr.sample_rate // len(base[0])
    return [np.tile(base[i % 16], reps) for i in range(n)]


def host_metrics(scores, thr):
    """what the reference's loop computes from the predictions of each recording"""
    rows, buckets = [], np.zeros(len(thr))
    for p in scores:
        det = TriggerDetector(CHUNK, trigger_level=0, sensitivity=THRESHOLD)
        rows.append((len(p), int((p > det.sensitivity).sum()), sum(det.update(x) for x in p.reshape(-1)), float(p.sum(dtype=np.float64))))
        buckets += (p.reshape((-1, 1)) > thr.reshape((1, -1))).sum(axis=0)
    return rows, buckets


def run(name, recs, runner, reps):
    thr = default_thresholds()
    eng = runner.engine

    def simulate():
        return runner.simulate(recs, CHUNK, THRESHOLD, thr)

    def evaluate():
        t0 = time.perf_counter()
        scores = runner.evaluate_clips(recs, CHUNK)
        t1 = time.perf_counter()
        return host_metrics(scores, thr), scores, t1 - t0

    def loop():
        # (evaluate takes float64 samples: the conversion is part of the existing path)
        scores = [runner.evaluate(r, CHUNK) for r in recs]
        return host_metrics(scores, thr), scores

    (m, b, _), ((rows_e, b_e), s_e, _), ((rows_l, b_l), s_l) = simulate(), evaluate(), loop()       # warm-up and check
    if not all(np.array_equal(x, y) for x, y in zip(s_e, s_l)):
        raise SystemExit('%s: evaluate_clips and the per-recording loop disagree' % name)
    if rows_e != rows_l or not np.array_equal(b_e, b_l) or not np.array_equal(b, b_l.astype(np.int64)):
        raise SystemExit('%s: the bucket counts disagree' % name)
    for row, want in zip(m, rows_l):
        if (int(row['n_windows']), int(row['activated_chunks']), int(row['activations'])) != want[:3] or \
                abs(float(row['activation_sum']) - want[3]) > 1e-9 * max(1.0, want[3]):
            raise SystemExit('%s: the metrics disagree: %r against %r' % (name, row, want))
    ts, te, ted, tl = [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); simulate(); ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); dev = evaluate()[2]; te.append(time.perf_counter() - t0); ted.append(dev)
        t0 = time.perf_counter(); loop(); tl.append(time.perf_counter() - t0)
    eng.set_timing(True)
    ev = [(simulate(), eng.last_timing())[1] for _ in range(reps)]
    eng.set_timing(False)
    med = lambda v: float(np.median(v))                        # noqa: E731
    s, e, d, l = med(ts), med(te), med(ted), med(tl)
    samples = int(sum(len(r) for r in recs))
    return {'recordings': len(recs), 'hours_of_audio': round(samples / pr.sample_rate / 3600, 3), 'windows': int(m['n_windows'].sum()),
            'activations': int(m['activations'].sum()), 'audio_MB_float32': round(4 * samples / 1e6, 1),
            'simulate_s': round(s, 5), 'evaluate_plus_host_s': round(e, 5), 'evaluate_device_part_s': round(d, 5), 'loop_s': round(l, 5),
            'loop_over_simulate': round(l / s, 2), 'evaluate_plus_host_over_simulate': round(e / s, 2),
            'simulate_minus_evaluate_device_part_ms': round((s - d) * 1e3, 3),
            'front_end_launch_ms_last_pass': round(med([x[0] for x in ev]), 4), 'network_launch_ms_last_pass': round(med([x[1] for x in ev]), 4),
            'simulate_s_all': [round(x, 5) for x in ts], 'evaluate_plus_host_s_all': [round(x, 5) for x in te],
            'evaluate_device_part_s_all': [round(x, 5) for x in ted], 'loop_s_all': [round(x, 5) for x in tl]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--workload', choices=('a', 'b', 'both'), default='both')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error('--reps must be at least 7 (the median of fewer repetitions is not reported)')
    base = base_signals()
    runner = HipRunner(weights=synth.make_weights())
    res = {'reps': args.reps, 'chunk_size': CHUNK, 'thresholds': 1000}
    if args.workload in ('a', 'both'):
        res['a_2048_recordings_5_to_20_s'] = run('a', workload_a(base), runner, args.reps)
    if args.workload in ('b', 'both'):
        res['b_16_recordings_of_10_min'] = run('b', workload_b(base), runner, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    runner.engine.close()


if __name__ == '__main__':
    main()
