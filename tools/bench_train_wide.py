"""One training step of a wide network (pe_trainer_create_wide) against the same step in torch autograd on
the same GPU: samples per second at 64, 128 and 256 units.

    python tools/bench_train_wide.py [--units 64 128 256] [--samples 20000] [--batch 5000] [--reps 7] [--warmup 3] [--out FILE]

29 x 13 features, a dataset of seeded samples resident on the device, batches of 5000 random rows, dropout 0.2, loss_bias 0.7,
RMSprop with the Keras defaults.  Both are timed with a host clock around whole steps (each step ends in a synchronous read of
its loss), after `warmup` discarded steps; median, minimum and maximum of `reps` repetitions are reported per width:

  * hip:        ``HipTrainer(wide=True).step`` -- gather, forward with tape, backward chain, gradient GEMM, reduction and update;
  * torch_gpu:  the same step in float32 torch autograd on the same GPU (tools/bench_train.py's torch_step_fn).

``mfma``: the products of a step that the contract asks for, 2 n T 3H ((F + H) forward + H backward chain + (F + H + 1) weight
gradients) = 2 n T 3H (2F + 3H + 1) floating-point operations (padding to the 16-wide MFMA tile not counted), over the median
step time, as a fraction of the fp32 MFMA peak bench.py prices configs[3] against (157.3 TFLOP/s).

One JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_train import EPS, LOSS_BIAS, LR, RATE, RHO, timed, torch_step_fn     # noqa: E402
from mycroft_precise_amd import synth                      # noqa: E402
from mycroft_precise_amd._lib import HipTrainer            # noqa: E402

MFMA_F32_PEAK_TFLOPS = 157.3        # bench.py: the dense fp32 matrix peak configs[3] is priced against
T, F = 29, 13


def step_flops(n, H):
    return 2.0 * n * T * 3 * H * (2 * F + 3 * H + 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--units', type=int, nargs='+', default=[64, 128, 256])
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
        weights = synth.make_weights(F, (H,))
        trainer = HipTrainer(weights, T, F, wide=True)
        trainer.set_data(x, y)
        counter = [0]

        def hip_step(idx):
            counter[0] += 1
            return trainer.step(idx, RATE, 1, counter[0], LOSS_BIAS, LR, RHO, EPS, 0)

        row = {}

        def report(name, times):
            med = float(np.median(times))
            row[name + '_step_ms'] = {'median': round(1e3 * med, 4), 'min': round(1e3 * min(times), 4), 'max': round(1e3 * max(times), 4)}
            row[name + '_samples_per_s'] = round(args.batch / med, 1)
            return med

        med = report('hip', timed(hip_step, batches, args.warmup, args.reps))
        trainer.close()
        tflops = step_flops(args.batch, H) / med / 1e12
        row['mfma'] = {'flop_per_step': step_flops(args.batch, H), 'achieved_tflops': round(tflops, 3),
                       'frac_of_peak': round(tflops / MFMA_F32_PEAK_TFLOPS, 4)}
        if torch.cuda.is_available():
            report('torch_gpu', timed(torch_step_fn(weights, x, y, 'cuda'), batches, args.warmup, args.reps))
            row['hip_over_torch_gpu'] = round(row['hip_samples_per_s'] / row['torch_gpu_samples_per_s'], 2)
        else:
            row['torch_gpu_samples_per_s'] = None       # unmeasured: torch sees no GPU
        res['widths'][str(H)] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
