"""Mel rows against MFCC rows through the same kernels: what one update costs on a Vectorizer.mels engine and on its MFCC twin.

    python tools/bench_mels.py [--out profiles/mels/bench_mels.json] [--reps 7] [--discard 3] [--launches 20]

Two engines live in ONE process and take turns, round by round, at 4096 streams, a 20-unit network and 1024-sample chunks:

  mels 20 filters     the default mels shape (n_fft 512, 20 filters): general front end, MELS instantiation, 32-float rows
  mfccs n_mfcc 20     the mfccs engine with 20 coefficients over the same 20 filters: the same general front end with its DCT
                      stage, the same 32-float rows, the same network shape (20 inputs, 20 units)

A round times, with HIP events, `launches` back-to-back updates (pe_update_device: front-end launch + network launch) on
warmed streams, per update; `discard` rounds are thrown away, then `reps` are kept: median and min - max.  The expectation is
only that dropping the DCT does not make the update slower than its MFCC twin; the tool prints and records both numbers and
gates nothing.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.params import pr, Vectorizer

STREAMS, UNITS, CHUNK = 4096, (20,), 1024
ENGINES = [('mels 20 filters', dict(vectorizer=Vectorizer.mels)), ('mfccs n_mfcc 20', dict(n_mfcc=20))]


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n          # ms


def stats(v):
    return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mels', 'bench_mels.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--discard', type=int, default=3)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--mfcc-precision', default='f64', choices=['f64', 'f32'])
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    pcm = (torch.randn((8, STREAMS, CHUNK), device=dev) * 3000).to(torch.int16)
    out = torch.zeros(STREAMS, device=dev)
    w = synth.make_weights(n_in=20, units=UNITS, seed=900)
    engs = {}
    for name, kw in ENGINES:
        hpr = pr.copy()
        hpr.__dict__.update(kw)
        e = engs[name] = _lib.HipEngine(hpr, w, n_streams=STREAMS, mfcc_precision=args.mfcc_precision)
        assert e.feature_size == 20
        for i in range(40):                # the windows fill
            e.update_device(pcm[i % 8].data_ptr(), CHUNK, out.data_ptr(), st)
    torch.cuda.synchronize()
    ms = {name: [] for name in engs}
    turn = [0]

    def one(e):
        turn[0] += 1
        e.update_device(pcm[turn[0] % 8].data_ptr(), CHUNK, out.data_ptr(), st)
    for r in range(args.discard + args.reps):
        for name, e in engs.items():
            t = timed(lambda: one(e), args.launches)
            if r >= args.discard:
                ms[name].append(t)
    for e in engs.values():
        e.close()
    rows = []
    base = float(np.median(ms['mfccs n_mfcc 20']))
    for name, _ in ENGINES:
        row = {'engine': name, 'streams': STREAMS, 'units': list(UNITS), 'chunk': CHUNK, 'mfcc_precision': args.mfcc_precision,
               'update_us': {k: 1e3 * v for k, v in stats(ms[name]).items()}, 'over_mfcc_twin': float(np.median(ms[name])) / base}
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump({'reps': args.reps, 'discard': args.discard, 'launches': args.launches, 'rows': rows}, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
