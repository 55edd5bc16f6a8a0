"""Wide / stacked networks: the bf16-operand kernel (gru_wide_bf16_device.h) against the float32 forms 0 and 2.

    python tools/bench_wide_bf16.py [--out profiles/wide_bf16/bench_wide_bf16.json] [--reps 7] [--discard 3] [--launches 20]

Per shape (256 x 2, 128, 64 units at 4096 and 65 536 streams) three engines live in ONE process and take turns, round by
round: float32 form 0, float32 form 2, bf16.  A round times, with HIP events,
  network   `launches` back-to-back pe_run_device calls on warmed windows (the network launch alone), per launch
  update    `launches` back-to-back pe_update_device calls (front end + network), per update
`discard` rounds are thrown away, then `reps` are kept: median and min - max.  Beside every network time stand the two bounds
it is priced against: the bf16 matrix peak and the weight stream from L2 at 64 B/clk/CU; `binds` names the larger.
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
from mycroft_precise_amd.params import pr

SHAPES = [(256, 256), (128,), (64,)]
STREAMS = [4096, 65536]
FORMS = [('f32 form 0', 'f32', 0), ('f32 form 2', 'f32', 2), ('bf16', 'bf16', 0)]
CLOCK_HZ, N_CUS = 2.4e9, 256                     # MI355X
BF16_DENSE_FLOPS = 2.5e15                        # v_mfma_f32_16x16x32_bf16: 16 x 16 x 32 x 2 flop in 8 cycles per SIMD -> 2048 flop/clk/SIMD
L2_BYTES_PER_CLK_CU = 64


def bounds(units, streams):
    """-> (seconds of bf16 matrix work, seconds of L2 weight stream) of one network launch of the bf16 kernel"""
    T, F = pr.n_features, 13
    Hp = (max(units) + 63) // 64 * 64
    tiles = (streams + 15) // 16
    macs = 0          # per window and timestep, padded as the kernel runs them (input part: one k-group of 32 for layer 1)
    wbytes = 0        # per workgroup and timestep
    for l in range(len(units)):
        kin = 32 if l == 0 else Hp
        macs += 3 * Hp * (kin + Hp)
        wbytes += 2 * 3 * Hp * (kin + Hp)
    flop = 2.0 * macs * 16 * tiles * T
    t_mfma = flop / BF16_DENSE_FLOPS
    rounds = -(-tiles // N_CUS)                 # workgroups a compute unit runs one after the other, if one is resident at a time
    t_l2 = wbytes * T * rounds / (L2_BYTES_PER_CLK_CU * CLOCK_HZ)
    return t_mfma, t_l2, wbytes


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n          # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'wide_bf16', 'bench_wide_bf16.json'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--discard', type=int, default=3)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--shapes', default='')      # e.g. "64;128" or "256,256"
    ap.add_argument('--streams', default='')
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(',')) for s in args.shapes.split(';')] if args.shapes else SHAPES
    streams_list = [int(s) for s in args.streams.split(',')] if args.streams else STREAMS
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for units in shapes:
        w = synth.make_weights(units=units, seed=900)
        for B in streams_list:
            pcm = (torch.randn((8, B, 1024), device=dev) * 3000).to(torch.int16)
            out = torch.zeros(B, device=dev)
            engs = []
            for name, prec, tiling in FORMS:
                e = _lib.HipEngine(pr, w, n_streams=B, gru_precision=prec)
                e.set_gru_tiling(tiling)
                for i in range(32):                                  # the windows fill
                    e.update_device(pcm[i % 8].data_ptr(), 1024, out.data_ptr(), st)
                engs.append(e)
            torch.cuda.synchronize()
            net = {name: [] for name, _, _ in FORMS}
            upd = {name: [] for name, _, _ in FORMS}
            k = [0]

            def one_update(e):
                e.update_device(pcm[k[0] % 8].data_ptr(), 1024, out.data_ptr(), st)
                k[0] += 1
            for r in range(args.discard + args.reps):
                for (name, _, _), e in zip(FORMS, engs):             # the forms alternate inside every round
                    n_ms = timed(lambda: e.run_device(out.data_ptr(), st), args.launches)
                    u_ms = timed(lambda: one_update(e), args.launches)
                    if r >= args.discard:
                        net[name].append(n_ms)
                        upd[name].append(u_ms)
            for e in engs:
                e.close()
            t_mfma, t_l2, wbytes = bounds(units, B)
            for name, _, _ in FORMS:
                row = {'units': list(units), 'streams': B, 'form': name,
                       'network_ms': {'median': float(np.median(net[name])), 'min': min(net[name]), 'max': max(net[name])},
                       'update_ms': {'median': float(np.median(upd[name])), 'min': min(upd[name]), 'max': max(upd[name])},
                       'windows_per_s': B / (1e-3 * float(np.median(net[name])))}
                if name == 'bf16':
                    row['bounds_ms'] = {'bf16_matrix_peak': 1e3 * t_mfma, 'l2_weight_stream_64B_per_clk_cu': 1e3 * t_l2,
                                        'weight_bytes_per_timestep_and_workgroup': wbytes,
                                        'binds': 'l2 weight stream' if t_l2 > t_mfma else 'bf16 matrix peak'}
                    row['speedup_over_f32_form0'] = float(np.median(net['f32 form 0'])) / float(np.median(net['bf16']))
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump({'reps': args.reps, 'discard': args.discard, 'launches': args.launches, 'rows': rows}, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
