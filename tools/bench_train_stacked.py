"""One training step of a stacked two-layer network (pe_trainer_create_stacked) against the same step in torch
autograd on the same GPU, and against the one-layer wide step at H = H1: samples per second at (64, 64), (128, 128), (256, 256).

    python tools/bench_train_stacked.py [--units 64 128 256] [--samples 20000] [--batch 5000] [--reps 7] [--warmup 3] [--out FILE]

29 x 13 features, a dataset of seeded samples resident on the device, batches of 5000 random rows, dropout 0.2 in both layers,
loss_bias 0.7, RMSprop with the Keras defaults.  All are timed with a host clock around whole steps (each step ends in a
synchronous read of its loss), after `warmup` discarded steps; median, minimum and maximum of `reps` repetitions per width:

  * hip:        ``HipTrainer(stacked=True).step`` -- gather, both forwards with tape, both backward chains, both gradient GEMMs,
                reduction and update;
  * torch_gpu:  the same step in float32 torch autograd on the same GPU;
  * hip_wide:   ``HipTrainer(wide=True).step`` of the one-layer network of H1 units (tools/bench_train_wide.py's step), same run.

``hip_over_torch_gpu`` is the project's bar (>= 1); ``hip_over_hip_wide`` (stacked step time over one-layer step time) is
reported, not gated.  ``mfma``: the products the contract asks for, per layer 2 n T 3H (2K + 3H + 1) with K the layer's input
width, plus layer 1's dx_t (2 n T 3 H1 H2), over the median step time, as a fraction of the fp32 MFMA peak (157.3 TFLOP/s).

One JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_train import EPS, LOSS_BIAS, LR, RATE, RHO, timed     # noqa: E402
from bench_train_wide import MFMA_F32_PEAK_TFLOPS, F, T           # noqa: E402
from mycroft_precise_amd import synth                      # noqa: E402
from mycroft_precise_amd._lib import HipTrainer            # noqa: E402


def layer_flops(n, K, H):
    return 2.0 * n * T * 3 * H * (2 * K + 3 * H + 1)


def step_flops(n, H1, H2):
    return layer_flops(n, F, H1) + layer_flops(n, H1, H2) + 2.0 * n * T * 3 * H1 * H2


def torch_step_fn(weights, x, y, device):
    """tools/bench_train.py's torch_step_fn for two GRU layers, each with its own per-gate masks"""
    import torch
    flat = [a for layer in weights['gru'] for a in layer]
    H2 = weights['gru'][1][1].shape[0]
    src = [(a, a.shape) for a in flat] + [(weights['dense_kernel'], (H2,)), (weights['dense_bias'], (1,))]
    params = [torch.tensor(np.asarray(a, dtype=np.float32).reshape(s), device=device, requires_grad=True) for a, s in src]
    opt = torch.optim.RMSprop(params, lr=LR, alpha=RHO, eps=EPS)
    xd, yd = torch.tensor(x, device=device), torch.tensor(y, device=device)
    keep = 1.0 / (1.0 - RATE)

    def layer(seq, W, U, bias):
        H = U.shape[0]
        m = (torch.rand((3, seq.shape[0], seq.shape[2]), device=device) >= RATE).to(seq.dtype) * keep
        h = torch.zeros((seq.shape[0], H), device=device)
        out = []
        for t in range(seq.shape[1]):
            xt = seq[:, t, :]
            z = torch.clamp(0.2 * ((xt * m[0]) @ W[:, :H] + bias[:H] + h @ U[:, :H]) + 0.5, 0.0, 1.0)
            r = torch.clamp(0.2 * ((xt * m[1]) @ W[:, H:2 * H] + bias[H:2 * H] + h @ U[:, H:2 * H]) + 0.5, 0.0, 1.0)
            c = (xt * m[2]) @ W[:, 2 * H:] + bias[2 * H:] + (r * h) @ U[:, 2 * H:]
            h = z * h + (1.0 - z) * c
            out.append(h)
        return torch.stack(out, dim=1)

    def step(idx):
        i = torch.as_tensor(idx, device=device, dtype=torch.long)
        xb, yb = xd.index_select(0, i), yd.index_select(0, i)
        h = layer(layer(xb, *params[0:3]), *params[3:6])[:, -1, :]
        p = torch.sigmoid(h @ params[6] + params[7])
        loss = LOSS_BIAS * (-(1.0 - yb) * torch.log(1.0 - p + 1e-7)).mean() + (1.0 - LOSS_BIAS) * (-yb * torch.log(p + 1e-7)).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return float(loss.detach())     # (a synchronous read, as the HIP step's loss is)
    return step


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--units', type=int, nargs='+', default=[64, 128, 256], help='H: the network is (H, H)')
    ap.add_argument('--samples', type=int, default=20000)
    ap.add_argument('--batch', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps must be at least 5 (the median of fewer repetitions is not reported)')
    import torch
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 1.0, (args.samples, T, F)).astype(np.float32)
    y = (rng.random(args.samples) < 0.5).astype(np.float32)
    batches = [rng.choice(args.samples, args.batch, replace=False).astype(np.int32) for _ in range(8)]
    res = {'samples': args.samples, 'batch': args.batch, 'reps': args.reps, 'warmup': args.warmup, 'features': [T, F],
           'mfma_peak_tflops': MFMA_F32_PEAK_TFLOPS, 'widths': {}}
    for H in args.units:
        weights = synth.make_weights(F, (H, H))
        row = {}

        def report(name, times):
            med = float(np.median(times))
            row[name + '_step_ms'] = {'median': round(1e3 * med, 4), 'min': round(1e3 * min(times), 4), 'max': round(1e3 * max(times), 4)}
            row[name + '_samples_per_s'] = round(args.batch / med, 1)
            return med

        def hip(trainer):
            trainer.set_data(x, y)
            counter = [0]

            def step(idx):
                counter[0] += 1
                return trainer.step(idx, RATE, 1, counter[0], LOSS_BIAS, LR, RHO, EPS, 0)
            times = timed(step, batches, args.warmup, args.reps)
            trainer.close()
            return times

        med = report('hip', hip(HipTrainer(weights, T, F, stacked=True)))
        wide = report('hip_wide', hip(HipTrainer(synth.make_weights(F, (H,)), T, F, wide=True)))
        row['hip_over_hip_wide'] = round(med / wide, 2)
        flops = step_flops(args.batch, H, H)
        tflops = flops / med / 1e12
        row['mfma'] = {'flop_per_step': flops, 'achieved_tflops': round(tflops, 3), 'frac_of_peak': round(tflops / MFMA_F32_PEAK_TFLOPS, 4)}
        if torch.cuda.is_available():
            report('torch_gpu', timed(torch_step_fn(weights, x, y, 'cuda'), batches, args.warmup, args.reps))
            row['hip_over_torch_gpu'] = round(row['hip_samples_per_s'] / row['torch_gpu_samples_per_s'], 2)
        else:
            row['torch_gpu_samples_per_s'] = None       # unmeasured: torch sees no GPU
        res['widths']['%dx%d' % (H, H)] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
