"""K models on one engine (pe_create_models) against K one-model engines: microseconds per update.

    python tools/gpu_multi_model.py [--steps 200] [--rounds 3] [--points 4096:1,4096:2,...]

One JSON line per point: K in {1, 2, 4, 8} x {4096, 65 536} streams with the float64 front end and the stock float32
network, plus the configs[4] shape (bf16 network and rows, float32 front end) at 65 536.  Timing as the bench headline:
HIP events around `steps` calls of pe_update_device_keep on two alternating resident slabs, after warm-up; the K-model
engine and the K one-model engines are timed alternately in the same process, `rounds` times, and the median is kept.
windows/s counts K x streams.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mycroft_precise_amd import synth                      # noqa: E402
from mycroft_precise_amd._lib import HipEngine             # noqa: E402
from mycroft_precise_amd.params import pr                  # noqa: E402

CHUNK = 1024


def time_updates(torch, engines, slabs, outs, steps, stream):
    """us per step, one step = one keep-update of every engine in `engines`"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(steps):
        for e, o in zip(engines, outs):
            e.update_device(slabs[i % 2].data_ptr(), CHUNK, o.data_ptr(), stream, keep=True)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / steps


def point(torch, n, K, gp, steps, rounds):
    dev = torch.device('cuda', 0)
    prec = dict(gru_precision='bf16', ring_precision='bf16', mfcc_precision='f32') if gp == 'bf16' else {}
    models = [synth.make_weights(seed=42 + k) for k in range(K)]
    multi = HipEngine(pr, models, n_streams=n, **prec)
    ones = [HipEngine(pr, w, n_streams=n, **prec) for w in models]
    base = synth.batch_pcm(256, 2)
    slabs = [torch.from_numpy(np.ascontiguousarray(np.tile(base[u], (n // 256, 1)))).to(dev) for u in range(2)]
    out_m = [torch.empty(K * n, device=dev)]
    out_1 = [torch.empty(n, device=dev) for _ in ones]
    st = torch.cuda.current_stream().cuda_stream
    time_updates(torch, [multi], slabs, out_m, 20, st)          # warm-up
    time_updates(torch, ones, slabs, out_1, 20, st)
    tm, t1 = [], []
    for _ in range(rounds):
        tm.append(time_updates(torch, [multi], slabs, out_m, steps, st))
        t1.append(time_updates(torch, ones, slabs, out_1, steps, st))
    m, s = float(np.median(tm)), float(np.median(t1))
    res = {'streams': n, 'models': K, 'network': 'bf16' if gp == 'bf16' else 'f32', 'front_end': 'f32' if gp == 'bf16' else 'f64',
           'form': multi.gru_tiling(), 'steps': steps, 'rounds': rounds,
           'us_per_update_k_model_engine': round(m, 2), 'us_per_update_k_engines': round(s, 2),
           'ratio': round(m / s, 3), 'k_model_us_all_rounds': [round(x, 2) for x in tm], 'k_engines_us_all_rounds': [round(x, 2) for x in t1],
           'windows_per_s_k_model_engine': round(K * n / (m * 1e-6)), 'windows_per_s_k_engines': round(K * n / (s * 1e-6))}
    for e in [multi] + ones:
        e.close()
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--points', default='4096:1,4096:2,4096:4,4096:8,65536:1,65536:2,65536:4,65536:8,65536:2:bf16')
    a = ap.parse_args()
    for p in a.points.split(','):
        f = p.split(':')
        print(json.dumps(point(torch, int(f[0]), int(f[1]), f[2] if len(f) > 2 else 'f32', a.steps, a.rounds)), flush=True)


if __name__ == '__main__':
    main()
