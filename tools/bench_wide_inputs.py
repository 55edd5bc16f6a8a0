"""Float32 wide / stacked networks: what the second layer-0 input k-group costs, and that the one-group path kept its time.

    python tools/bench_wide_inputs.py [--out profiles/wide_inputs/bench_wide_inputs.json] [--reps 7] [--discard 3] [--launches 20]
                                      [--parent-lib PATH/libprecise_engine.so]

Per shape ((64,), (128,), (256, 256) units at 4096 streams) and form (0: f32-input MFMAs, 2: float32 products on the bf16
pipe) three engines live in ONE process and take turns, round by round: 13 plain inputs, 26 inputs (use_delta), 20
coefficients.  A round times, with HIP events, `launches` back-to-back pe_run_device calls on warmed windows (the network
launch alone), per launch.  `discard` rounds are thrown away, then `reps` are kept: median and min - max.  Beside every
time stands the MFMA work counted from the shapes: k-groups of 16 per output tile and timestep (the second input group adds
one to layer 0's 1 + H/16), and the multiply-adds of a launch.

--parent-lib: a build of the library from the parent commit.  At (256, 256) and (64,), forms 0 and 2, the plain 13-input
engine of that library and of this tree alternate in the same rounds; the medians must not differ by more than the spread
(min - max over the kept rounds) the parent's own library shows in that call (`within_parent_spread`).
"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.params import pr

SHAPES = [(64,), (128,), (256, 256)]
AB_SHAPES = [(256, 256), (64,)]
STREAMS = 4096
FORMS = [0, 2]
INPUTS = [('13 plain', 13, {}), ('26 use_delta', 26, dict(use_delta=True)), ('20 coefficients', 20, dict(n_fft=1024, n_filt=40, n_mfcc=20))]


def work(units, n_in, streams):
    """-> (k-groups of 16 per output tile and timestep in layer 0, in the whole network; multiply-adds of one launch, padded
    as the kernel runs them)"""
    T = pr.n_features
    Hp = (max(units) + 63) // 64 * 64
    kx = 2 if n_in > 16 else 1
    groups0 = kx + Hp // 16
    groups = groups0 + (len(units) - 1) * 2 * (Hp // 16)
    macs = 3 * Hp * 16 * groups * T * ((streams + 15) // 16 * 16)
    return groups0, groups, macs


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n          # ms


def bind(path):
    """another build of the library, bound like _lib.load() binds the in-tree one"""
    lib = C.CDLL(path)
    for name, (res, args) in _lib.EXPORTS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.pe_abi_version() == _lib.ABI_VERSION
    return lib


def make_engine(lib, kw, w, streams, tiling, pcm, out, st):
    hpr = pr.copy()
    hpr.__dict__.update(kw)
    tree = _lib.load()
    _lib._lib = lib                       # HipEngine keeps the library it was created with
    try:
        e = _lib.HipEngine(hpr, w, n_streams=streams)
    finally:
        _lib._lib = tree
    e.set_gru_tiling(tiling)
    for i in range(32):                   # the windows fill
        e.update_device(pcm[i % 8].data_ptr(), 1024, out.data_ptr(), st)
    return e


def rounds(engs, out, st, args):
    """{name: [ms per launch of each kept round]}: the engines alternate inside every round"""
    ms = {name: [] for name in engs}
    for r in range(args.discard + args.reps):
        for name, e in engs.items():
            t = timed(lambda: e.run_device(out.data_ptr(), st), args.launches)
            if r >= args.discard:
                ms[name].append(t)
    return ms


def stats(v):
    return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'wide_inputs', 'bench_wide_inputs.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--discard', type=int, default=3)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--parent-lib', default='')
    args = ap.parse_args()
    import warnings
    warnings.simplefilter('ignore')
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    tree = _lib.load()
    pcm = (torch.randn((8, STREAMS, 1024), device=dev) * 3000).to(torch.int16)
    out = torch.zeros(STREAMS, device=dev)
    rows, ab = [], []
    for units in SHAPES:
        for tiling in FORMS:
            engs = {name: make_engine(tree, kw, synth.make_weights(n_in=n_in, units=units, seed=900), STREAMS, tiling, pcm, out, st)
                    for name, n_in, kw in INPUTS}
            torch.cuda.synchronize()
            ms = rounds(engs, out, st, args)
            for e in engs.values():
                e.close()
            base = float(np.median(ms['13 plain']))
            for name, n_in, _ in INPUTS:
                g0, g, macs = work(units, n_in, STREAMS)
                row = {'units': list(units), 'streams': STREAMS, 'form': tiling, 'inputs': name, 'network_ms': stats(ms[name]),
                       'over_13_plain': float(np.median(ms[name])) / base,
                       'kgroups_layer0': g0, 'kgroups_network': g, 'kgroups_over_13_plain': g / work(units, 13, STREAMS)[1], 'macs_per_launch': macs}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.parent_lib:
        parent = bind(os.path.abspath(args.parent_lib))
        for units in AB_SHAPES:
            for tiling in FORMS:
                w = synth.make_weights(n_in=13, units=units, seed=900)
                engs = {'parent': make_engine(parent, {}, w, STREAMS, tiling, pcm, out, st),
                        'tree': make_engine(tree, {}, w, STREAMS, tiling, pcm, out, st)}
                torch.cuda.synchronize()
                ms = rounds(engs, out, st, args)
                for e in engs.values():
                    e.close()
                p, t = stats(ms['parent']), stats(ms['tree'])
                spread = p['max'] - p['min']
                row = {'units': list(units), 'streams': STREAMS, 'form': tiling, 'inputs': '13 plain', 'parent_ms': p, 'tree_ms': t,
                       'parent_spread_ms': spread, 'median_difference_ms': t['median'] - p['median'],
                       'within_parent_spread': bool(abs(t['median'] - p['median']) <= spread)}
                ab.append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump({'reps': args.reps, 'discard': args.discard, 'launches': args.launches, 'rows': rows, 'parent_against_tree': ab}, f, indent=1)
        f.write('\n')
    if any(not r['within_parent_spread'] for r in ab):
        sys.exit('the plain 13-input launch differs from the parent build by more than the parent\'s own spread')


if __name__ == '__main__':
    main()
