#!/usr/bin/env python3
"""Chain launch, us per update by HIP events (profiles/chain_launch/README.md): back-to-back pe_update_device /
pe_update_subset_device over a 25-slab cycle of resident PCM, carried chains eager, best of 3.  One library per process: name
another build with PE_LIB (mycroft_precise_amd/_lib.py) and let the variants take turns.

    [PE_LIB=/path/to/libprecise_engine.so] python tools/bench_chain_launch.py LABEL [--b8192] [--n 2500] [--chunk 1024]

Prints one line per batch size: full update, and at 4096 streams a subset naming all streams and a quarter subset.  --chunk:
samples per stream and update (the first samples of every 1024-sample slab; 800 = one hop: no chain is ever left out)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mycroft_precise_amd import synth, params as P          # noqa: E402
from mycroft_precise_amd._lib import HipEngine              # noqa: E402

label = sys.argv[1]
N = int(sys.argv[sys.argv.index('--n') + 1]) if '--n' in sys.argv else 2500
CHUNK = int(sys.argv[sys.argv.index('--chunk') + 1]) if '--chunk' in sys.argv else 1024
assert 1 <= CHUNK <= 1024
dev = torch.device('cuda', 0)
st = torch.cuda.current_stream().cuda_stream
w = synth.make_weights()
n_res = 25                  # updates of 1024 samples after which the pattern of new frames and new rows repeats


def slabs(B):
    base = synth.batch_pcm(64, n_res)[:, :, :CHUNK]                             # [25][64][CHUNK]
    return torch.from_numpy(np.ascontiguousarray(np.tile(base, (1, B // 64, 1)))).to(dev)


def timed(fn, n):
    best = 1e9
    for rep in range(3):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for i in range(n):
            fn(i)
        ev1.record(); ev1.synchronize()
        best = min(best, ev0.elapsed_time(ev1) / n * 1e3)
    return best


def run(B):
    pcm = slabs(B)
    e = HipEngine(P.pr, w, n_streams=B)
    e.set_chain_carry(2)
    out = torch.zeros(B, device=dev)

    def full(i):
        e.update_device(pcm[i % n_res].data_ptr(), CHUNK, out.data_ptr(), st)
    for i in range(500):
        full(i)
    torch.cuda.synchronize()
    assert e.chain_carry() == (2, True)
    res = {'full': timed(full, N)}
    if B == 4096:
        ids = torch.arange(B, dtype=torch.int32, device=dev)

        def sub(i):
            e.update_subset_device(ids.data_ptr(), B, pcm[i % n_res].data_ptr(), CHUNK, out.data_ptr(), st)
        for i in range(200):
            sub(i)
        res['subset_all'] = timed(sub, N)
        some = torch.arange(0, B, 4, dtype=torch.int32, device=dev)
        part = pcm[:, ::4].contiguous()
        osome = torch.zeros(B // 4, device=dev)

        def quarter(i):
            e.update_subset_device(some.data_ptr(), B // 4, part[i % n_res].data_ptr(), CHUNK, osome.data_ptr(), st)
        for i in range(200):
            quarter(i)
        res['quarter'] = timed(quarter, N)
    torch.cuda.synchronize()
    assert e.chain_carry() == (2, True)
    s = float(out.double().nan_to_num().sum())
    e.close()
    return res, s


for B in ([4096] + ([8192] if '--b8192' in sys.argv else [])):
    res, s = run(B)
    print('AB %-10s B %d chunk %d ' % (label, B, CHUNK) + ' '.join('%s %.2f' % kv for kv in res.items()) + ' us  sum %.6f' % s, flush=True)
