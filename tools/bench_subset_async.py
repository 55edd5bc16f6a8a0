"""Host-fed updates for streams that advance on their own (pe_update_subset_async) against the calls that exist without it.

    python tools/bench_subset_async.py [--streams 4096] [--chunk 1024] [--updates 2000] [--reps 7] [--out FILE] [--baseline-only]

4096 streams of the stock model, chunks of 1024 samples in pe_host_alloc'ed (pinned) buffers, results into pinned buffers.
Every figure is microseconds per update: a host clock around `updates` calls that end in pe_wait (pipelined calls) or that
each end in their own synchronous copy back (pe_update_subset), after a warm-up of the same calls; the variants of one
comparison are timed alternately in the same process and the median of `reps` repetitions is kept, with the spread
(min .. max) beside it.

  (a) every stream:  pe_update_subset_async(ids = NULL), and the same with an explicit list of every id, against
                     pe_update_async -- the same update; the list adds 16 KB of ids to the 8 MB of audio.
  (b) a random half of the streams per call (a fresh draw every call, ids sorted): pe_update_subset_async against a loop of
                     synchronous pe_update_subset from the same pinned buffers.
  (c) as (b), with conf and fired asked for: pe_update_subset_async(conf, fired) against pe_update_subset followed by
                     pe_decode_subset.

Before anything is timed the pipelined results of one pass are compared bit for bit with the synchronous ones.
--baseline-only times pe_update_async alone (what an older library can run).  One JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mycroft_precise_amd import synth                                  # noqa: E402
from mycroft_precise_amd._lib import HipEngine                         # noqa: E402
from mycroft_precise_amd.params import pr                              # noqa: E402
from mycroft_precise_amd.threshold_decoder import ThresholdDecoder     # noqa: E402

DEPTH = 4          # pinned buffers per role: three updates in flight and the one being filled


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--streams', type=int, default=4096)
    ap.add_argument('--chunk', type=int, default=1024)
    ap.add_argument('--updates', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--baseline-only', action='store_true')
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps must be at least 5 (the median of fewer repetitions is not reported)')
    n, chunk, n_up = args.streams, args.chunk, args.updates
    half = n // 2
    rng = np.random.default_rng(11)

    def engine():
        e = HipEngine(pr, synth.make_weights(), n_streams=n)
        e.set_decoder(ThresholdDecoder(pr.threshold_config, pr.threshold_center))
        e.set_trigger(2 * chunk, 0.5, 3)
        return e
    eng = engine()
    base = synth.batch_pcm(min(n, 64), DEPTH, chunk)                    # [DEPTH][<= 64][chunk], tiled over the streams
    pcm = [eng.host_array((n, chunk), '<i2') for _ in range(DEPTH)]
    for i, p in enumerate(pcm):
        p[...] = base[i][np.arange(n) % base.shape[1]]
    raw = [eng.host_array((n,), np.float32) for _ in range(DEPTH)]
    conf = [eng.host_array((n,), np.float64) for _ in range(DEPTH)]
    fired = [eng.host_array((n,), np.uint8) for _ in range(DEPTH)]
    every = np.arange(n, dtype=np.int32)
    halves = [np.sort(rng.permutation(n)[:half]).astype(np.int32) for _ in range(n_up)]

    def full_async():
        for u in range(n_up):
            eng.update_async(pcm[u % DEPTH], raw[u % DEPTH])
        eng.wait()

    def all_null():
        for u in range(n_up):
            eng.update_subset_async(None, pcm[u % DEPTH], raw[u % DEPTH])
        eng.wait()

    def all_ids():
        for u in range(n_up):
            eng.update_subset_async(every, pcm[u % DEPTH], raw[u % DEPTH])
        eng.wait()

    def half_async():
        for u in range(n_up):
            eng.update_subset_async(halves[u], pcm[u % DEPTH][:half], raw[u % DEPTH][:half])
        eng.wait()

    def half_sync():
        for u in range(n_up):
            eng.update_subset(halves[u], pcm[u % DEPTH][:half])

    def half_async_detect():
        for u in range(n_up):
            i = u % DEPTH
            eng.update_subset_async(halves[u], pcm[i][:half], raw[i][:half], conf[i][:half], fired[i][:half])
        eng.wait()

    def half_sync_detect():
        for u in range(n_up):
            eng.decode_subset(halves[u], eng.update_subset(halves[u], pcm[u % DEPTH][:half]), want_fired=True)

    def check():
        """one pass of (c) on two fresh engines: the pipeline's three outputs against the synchronous calls', bit for bit"""
        a, b = engine(), engine()
        got = []
        for u in range(8):
            r, c, f = np.empty(half, np.float32), np.empty(half, np.float64), np.empty(half, np.uint8)
            b.update_subset_async(halves[u], pcm[u % DEPTH][:half], r, c, f)
            got.append((r, c, f))
        b.wait()
        for u, (r, c, f) in enumerate(got):
            wr = a.update_subset(halves[u], pcm[u % DEPTH][:half])
            wc, wf = a.decode_subset(halves[u], wr, want_fired=True)
            if not (np.array_equal(r, wr) and np.array_equal(c, wc) and np.array_equal(f.astype(bool), wf)):
                raise SystemExit('the pipeline and the synchronous calls disagree in update %d: nothing was timed' % u)
        a.close()
        b.close()

    groups = [('a', [('pe_update_async', full_async)])] if args.baseline_only else [
        ('a', [('pe_update_async', full_async), ('subset_async_null_ids', all_null), ('subset_async_every_id', all_ids)]),
        ('b', [('subset_async_half', half_async), ('update_subset_loop_half', half_sync)]),
        ('c', [('subset_async_half_conf_fired', half_async_detect), ('update_subset_decode_subset_loop_half', half_sync_detect)]),
    ]
    if not args.baseline_only:
        check()
    result = {'streams': n, 'chunk': chunk, 'updates_per_repetition': n_up, 'repetitions': args.reps, 'unit': 'us per update'}
    for tag, variants in groups:
        times = {name: [] for name, _ in variants}
        for name, fn in variants:
            fn()                                                         # warm-up of every shape the timed window uses
        for _ in range(args.reps):
            for name, fn in variants:                                    # alternately, in the same process
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) / n_up * 1e6)
        result[tag] = {name: {'median': round(float(np.median(t)), 2), 'min': round(min(t), 2), 'max': round(max(t), 2)}
                       for name, t in times.items()}
    if not args.baseline_only:
        med = lambda tag, name: result[tag][name]['median']             # noqa: E731
        result['ratios'] = {
            'a_null_ids_over_update_async': round(med('a', 'subset_async_null_ids') / med('a', 'pe_update_async'), 4),
            'a_every_id_over_update_async': round(med('a', 'subset_async_every_id') / med('a', 'pe_update_async'), 4),
            'b_loop_over_pipeline': round(med('b', 'update_subset_loop_half') / med('b', 'subset_async_half'), 4),
            'c_loop_over_pipeline': round(med('c', 'update_subset_decode_subset_loop_half') / med('c', 'subset_async_half_conf_fired'), 4),
        }
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
