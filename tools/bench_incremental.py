"""One incremental-training session (mining.Miner + train.IncrementalTrainer) against the loop a user writes without them.

    python tools/bench_incremental.py [--minutes 20] [--recordings 40] [--chunk 2048] [--delay 10] [--quantile 0.98] [--out FILE]

Synthetic not-wake-word audio (synth.stream_pcm as load_audio returns it: k / 32767 in float32), a random 20-unit network,
2000 seeded training windows.  The threshold is the `quantile` of the predictions of the untrained network over all chunks, so
that the session retrains a realistic number of times.  Both sides run the policy of scripts/train_incremental.py:113-137 on
the same recordings, flags and initial state, one after the other in this process, each after a warm-up at a small size:

  * session:  IncrementalTrainer.run -- scans on the device, hits appended device to device, fit_resident, set_weights;
  * loop:     Listener.update_raw per chunk, a host ring, vectorize_clips of the saved rings, Trainer.fit with a new upload of
              the whole set, and a new HipRunner per retrain.

Times are a host clock around each whole run (every step of both ends in a synchronous read).  One JSON line with both times,
the counts and whether the two hit lists and final weights are equal; --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mycroft_precise_amd import synth                                   # noqa: E402
from mycroft_precise_amd.mining import Miner                            # noqa: E402
from mycroft_precise_amd.model import ModelParams, save_weights         # noqa: E402
from mycroft_precise_amd.network_runner import HipRunner, Listener      # noqa: E402
from mycroft_precise_amd.params import pr                               # noqa: E402
from mycroft_precise_amd.train import IncrementalTrainer, Trainer       # noqa: E402
from mycroft_precise_amd.util import chunk_audio                        # noqa: E402

BATCH, EPOCHS, SEED = 5000, 1, 5


def make_inputs(minutes, n_rec, seed):
    rng = np.random.default_rng(seed)
    total = int(minutes * 60 * pr.sample_rate)
    cuts = np.sort(rng.integers(0, total, n_rec - 1))
    lengths = np.diff(np.concatenate(([0], cuts, [total])))
    audios = [synth.stream_pcm(s, int(n)).astype(np.float32) / np.float32(32767.0) for s, n in enumerate(lengths)]
    flags = [bool(v) for v in rng.random(n_rec) > 0.8]                  # train_incremental.py:115
    x = rng.normal(0.0, 1.0, (2000, pr.n_features, pr.feature_size)).astype(np.float32)
    y = (rng.random(2000) < 0.5).astype(np.float32)
    return audios, flags, x, y


def run_session(weights, audios, flags, x, y, chunk, delay, threshold):
    runner = HipRunner(weights=weights)
    trainer = Trainer(weights, ModelParams(recurrent_units=20), seed=SEED)
    t0 = time.perf_counter()
    trainer.set_data(x, y)
    inc = IncrementalTrainer(trainer, runner, delay_samples=delay, epochs=EPOCHS, batch_size=BATCH, threshold=threshold,
                             chunk_size=chunk, shuffle=False)
    hits, retrains = inc.run(audios, test_flags=flags)
    flat = trainer._t.get_weights()
    return time.perf_counter() - t0, hits, retrains, flat


def run_loop(model_file, weights, audios, flags, x, y, chunk, delay, threshold):
    lis = Listener(model_file, chunk)
    trainer = Trainer(weights, ModelParams(recurrent_units=20), seed=SEED)
    T, F, B = pr.n_features, pr.n_mfcc, pr.buffer_samples
    t0 = time.perf_counter()
    ring = np.zeros(B, dtype=np.float64)
    count, hits, retrains, train_rings, test_rings = 0, [], [], [], []
    for r, audio in enumerate(audios):
        lis.clear()
        for i, piece in enumerate(chunk_audio(audio, chunk)):
            ring = np.concatenate((ring[len(piece):], piece))[-B:]
            if lis.update_raw(piece) > threshold:
                count += 1
                hits.append((r, i, flags[r]))
                saved = (ring * 32767.0).astype(np.int16).astype(np.float32) / np.float32(32767.0)      # util.py:65,71
                (test_rings if flags[r] else train_rings).append(saved)
            if not flags[r] and count >= delay and EPOCHS > 0:
                count = 0
                retrains.append((r, i))
                new = lis._engine.vectorize_clips(train_rings, pr.max_samples).astype(np.float32).reshape(-1, T, F)
                val = lis._engine.vectorize_clips(test_rings, pr.max_samples).astype(np.float32).reshape(-1, T, F)
                trainer.fit(np.concatenate([x, new]), np.concatenate([y, np.zeros(len(new), np.float32)]), batch_size=BATCH,
                            epochs=EPOCHS, shuffle=False,
                            validation_data=(val, np.zeros(len(val), np.float32)) if len(val) else None)
                lis.runner = HipRunner(weights=trainer.weights)
    flat = trainer._t.get_weights()
    return time.perf_counter() - t0, hits, retrains, flat


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--minutes', type=float, default=20.0)
    ap.add_argument('--recordings', type=int, default=40)
    ap.add_argument('--chunk', type=int, default=2048)
    ap.add_argument('--delay', type=int, default=10)
    ap.add_argument('--quantile', type=float, default=0.98)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    weights = synth.make_weights(pr.n_mfcc, (20,), seed=7)
    model_file = os.path.join(tempfile.mkdtemp(prefix='bench_incremental_'), 'random20.npz')
    save_weights(model_file, weights)

    def both(minutes, n_rec, quantile):
        audios, flags, x, y = make_inputs(minutes, n_rec, seed=3)
        probe = Miner(HipRunner(weights=weights), audios, chunk_size=args.chunk)
        _, _, scores = probe.scan(return_scores=True)
        probe.close()
        threshold = float(np.quantile(scores.astype(np.float64), quantile))
        a = run_session(weights, audios, flags, x, y, args.chunk, args.delay, threshold)
        b = run_loop(model_file, weights, audios, flags, x, y, args.chunk, args.delay, threshold)
        return scores.size, threshold, a, b

    both(0.5, 3, 0.5)                                                   # warm-up: every code path of both sides, retrains included
    n_chunks, threshold, (ts, hs, rs, ws), (tl, hl, rl, wl) = both(args.minutes, args.recordings, args.quantile)
    res = {'minutes': args.minutes, 'recordings': args.recordings, 'chunk': args.chunk, 'delay_samples': args.delay,
           'chunks': int(n_chunks), 'threshold': threshold, 'hits': len(hs), 'retrains': len(rs),
           'session_s': round(ts, 4), 'loop_s': round(tl, 4), 'loop_over_session': round(tl / ts, 2),
           'hits_equal': hs == hl and rs == rl, 'weights_equal': ws.tobytes() == wl.tobytes()}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
