#!/usr/bin/env python3
"""Kernel trace of the headline loop with carried chains, split by update phase (profiles/chain_launch/README.md).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/trace_chain_launch.py loop [N]
    python tools/trace_chain_launch.py split LABEL DIR [DROP]

loop: 4096 streams, chains entered eagerly, N (600) pe_update_device_keep calls of 1024 samples over 25 resident slabs.
split: the durations of the fused_update_chains_kernel launches of such a trace (the first DROP = 100 dropped; 200 and N = 700 to
look only at launches that leave chains out, which begin after 128 calls: profiles/chain_skip/README.md), grouped by how many
frames and how many visible rows the update completes per stream -- counted from the sample positions, all streams being in
phase."""
import csv
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mycroft_precise_amd import params as P          # noqa: E402


def loop(N=600):
    import torch
    from mycroft_precise_amd import synth
    from mycroft_precise_amd._lib import HipEngine
    B, n_res = 4096, 25
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    base = synth.batch_pcm(64, n_res)
    pcm = torch.from_numpy(np.ascontiguousarray(np.tile(base, (1, B // 64, 1)))).to(dev)
    e = HipEngine(P.pr, synth.make_weights(), n_streams=B)
    e.set_chain_carry(2)
    out = torch.zeros(B, device=dev)
    for i in range(N):
        e.update_device(pcm[i % n_res].data_ptr(), 1024, out.data_ptr(), st, keep=True)
    torch.cuda.synchronize()
    assert e.chain_carry() == (2, True)
    print('trace loop done', float(out.sum()))
    e.close()


def split(label, d, drop=100):
    rows = []
    for f in glob.glob(d + '/**/*kernel_trace.csv', recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
    rows.sort()
    ch = [(e - s) / 1e3 for s, e, n in rows if 'fused_update_chains_kernel' in n]
    hop, win, flen = P.pr.hop_samples, P.pr.window_samples, min(P.pr.window_samples, P.pr.n_fft)

    def kc(p):
        return 0 if p < flen else 1 + (p - flen) // hop

    def ke(p):
        return 0 if p < win else 1 + (p - win) // hop
    phase = {}
    for u, t in enumerate(ch):
        if u >= drop:
            phase.setdefault((kc((u + 1) * 1024) - kc(u * 1024), ke((u + 1) * 1024) - ke(u * 1024)), []).append(t)
    print('TRACE %s: %d chain launches, all after the first %d: mean %.2f us median %.2f us' % (label, len(ch), drop, np.mean(ch[drop:]), np.median(ch[drop:])))
    for key in sorted(phase):
        v = phase[key]
        print('TRACE %s: frames %d rows %d: n %3d (%.0f %%) mean %.2f median %.2f min %.2f max %.2f us' %
              (label, key[0], key[1], len(v), 100.0 * len(v) / (len(ch) - drop), np.mean(v), np.median(v), min(v), max(v)))
    for s, e, n in rows:
        if 'gru_chains_rebuild_kernel' in n:
            print('TRACE %s: gru_chains_rebuild_kernel %.2f us' % (label, (e - s) / 1e3))


if __name__ == '__main__':
    if sys.argv[1] == 'loop':
        loop(*[int(x) for x in sys.argv[2:3]])
    else:
        split(sys.argv[2], sys.argv[3], *[int(x) for x in sys.argv[4:5]])
