"""One training step (pe_trainer_step) against the same step in torch autograd: samples per second.

    python tools/bench_train.py [--samples 50000] [--batch 5000] [--reps 7] [--warmup 3] [--cpu-reps 5] [--out FILE]

Stock shape (29 x 13 features, 20 units), a dataset of 50 000 seeded samples resident on the device, batches of 5000 random
rows, dropout 0.2, loss_bias 0.7, RMSprop with the Keras defaults.  Three things are timed with a host clock around whole
steps (each step ends in a synchronous read of its loss), after `warmup` discarded steps; median, minimum and maximum of
`reps` repetitions are reported:

  * hip:        ``HipTrainer.step`` -- gather, forward, backward, reduction and update in two launches;
  * torch_gpu:  the same step in float32 torch autograd on the same GPU (index_select, the GRU loop of DESIGN.md 4.9 with
                per-gate dropout masks drawn by torch, weighted_log_loss, backward, torch.optim.RMSprop);
  * torch_cpu:  the same torch code on the CPU.

One JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mycroft_precise_amd import synth                      # noqa: E402
from mycroft_precise_amd._lib import HipTrainer            # noqa: E402

RATE, LOSS_BIAS, LR, RHO, EPS = 0.2, 0.7, 1e-3, 0.9, 1e-7


def torch_step_fn(weights, x, y, device):
    import torch
    (k, rk, b), = weights['gru']
    H = rk.shape[0]
    params = [torch.tensor(np.asarray(a, dtype=np.float32).reshape(s), device=device, requires_grad=True)
              for a, s in ((k, k.shape), (rk, rk.shape), (b, b.shape), (weights['dense_kernel'], (H,)), (weights['dense_bias'], (1,)))]
    opt = torch.optim.RMSprop(params, lr=LR, alpha=RHO, eps=EPS)
    xd, yd = torch.tensor(x, device=device), torch.tensor(y, device=device)
    keep = 1.0 / (1.0 - RATE)

    def step(idx):
        W, U, bias, wd, bd = params
        i = torch.as_tensor(idx, device=device, dtype=torch.long)
        xb, yb = xd.index_select(0, i), yd.index_select(0, i)
        m = (torch.rand((3, xb.shape[0], xb.shape[2]), device=device) >= RATE).to(xb.dtype) * keep
        h = torch.zeros((xb.shape[0], H), device=device)
        for t in range(xb.shape[1]):
            xt = xb[:, t, :]
            z = torch.clamp(0.2 * ((xt * m[0]) @ W[:, :H] + bias[:H] + h @ U[:, :H]) + 0.5, 0.0, 1.0)
            r = torch.clamp(0.2 * ((xt * m[1]) @ W[:, H:2 * H] + bias[H:2 * H] + h @ U[:, H:2 * H]) + 0.5, 0.0, 1.0)
            c = (xt * m[2]) @ W[:, 2 * H:] + bias[2 * H:] + (r * h) @ U[:, 2 * H:]
            h = z * h + (1.0 - z) * c
        p = torch.sigmoid(h @ wd + bd)
        loss = LOSS_BIAS * (-(1.0 - yb) * torch.log(1.0 - p + 1e-7)).mean() + (1.0 - LOSS_BIAS) * (-yb * torch.log(p + 1e-7)).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return float(loss.detach())     # (a synchronous read, as the HIP step's loss is)
    return step


def timed(step, batches, warmup, reps):
    for i in range(warmup):
        step(batches[i % len(batches)])
    out = []
    for i in range(reps):
        t0 = time.perf_counter()
        step(batches[(warmup + i) % len(batches)])
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--samples', type=int, default=50000)
    ap.add_argument('--batch', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cpu-reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if min(args.reps, args.cpu_reps) < 5:
        ap.error('--reps and --cpu-reps must be at least 5 (the median of fewer repetitions is not reported)')
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 1.0, (args.samples, 29, 13)).astype(np.float32)
    y = (rng.random(args.samples) < 0.5).astype(np.float32)
    batches = [rng.choice(args.samples, args.batch, replace=False).astype(np.int32) for _ in range(8)]
    weights = synth.make_weights()

    trainer = HipTrainer(weights, 29, 13)
    trainer.set_data(x, y)
    counter = [0]

    def hip_step(idx):
        counter[0] += 1
        return trainer.step(idx, RATE, 1, counter[0], LOSS_BIAS, LR, RHO, EPS, 0)

    res = {'samples': args.samples, 'batch': args.batch, 'reps': args.reps, 'warmup': args.warmup, 'shape': [29, 13, 20]}

    def report(name, times):
        med = float(np.median(times))
        res[name + '_step_ms'] = {'median': round(1e3 * med, 4), 'min': round(1e3 * min(times), 4), 'max': round(1e3 * max(times), 4)}
        res[name + '_samples_per_s'] = round(args.batch / med, 1)

    report('hip', timed(hip_step, batches, args.warmup, args.reps))
    trainer.close()
    import torch
    if torch.cuda.is_available():
        report('torch_gpu', timed(torch_step_fn(weights, x, y, 'cuda'), batches, args.warmup, args.reps))
        res['hip_over_torch_gpu'] = round(res['hip_samples_per_s'] / res['torch_gpu_samples_per_s'], 2)
    else:
        res['torch_gpu_samples_per_s'] = None           # unmeasured: torch sees no GPU
    report('torch_cpu', timed(torch_step_fn(weights, x, y, 'cpu'), batches, 1, args.cpu_reps))
    res['torch_cpu_threads'] = torch.get_num_threads()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
