"""
Float64 reference for the training kernels.  TEST INFRASTRUCTURE ONLY.

The forward pass of ``oracle/keras_gru.py`` K1-K8 with the training-time input dropout of Keras 2.2.4 ``GRUCell``
(implementation 1: one mask per gate, the same for every timestep, multiplying x_t before that gate's input product), the
reference's ``weighted_log_loss`` (functions.py:47-50) and gradients by torch autograd, all in float64 on the CPU (``dtype``
may be lowered to float32 to measure the float32 floor).  It also returns every gate pre-activation and the logit, from which
the tests pick kink-safe samples: the hard sigmoid has kinks at pre-activation +-2.5, and a float32 kernel may legitimately
land on the other side of one.
"""
import numpy as np
import torch

NAMES = ('kernel', 'recurrent_kernel', 'bias', 'dense_kernel', 'dense_bias')
EPS = 1e-7


def tensors(weights, dtype=torch.float64, requires_grad=True):
    (k, rk, b), = weights['gru']
    src = [k, rk, b, np.asarray(weights['dense_kernel']).reshape(-1), np.asarray(weights['dense_bias']).reshape(-1)]
    # (float32 weights are widened exactly; a narrower dtype rounds them)
    return [torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype, requires_grad=requires_grad) for a in src]


def forward(params, x, masks=None):
    """x [N, T, F], masks [3, N, F] or None -> dict(p [N], logit [N], a_z / a_r [T, N, H])."""
    W, U, b, wd, bd = params
    H = U.shape[0]
    x = torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=W.dtype)
    n, T, _ = x.shape
    if masks is None:
        m = [None, None, None]
    else:
        m = [torch.as_tensor(np.asarray(g, dtype=np.float64), dtype=W.dtype) for g in masks]
    Wz, Wr, Wh = W[:, :H], W[:, H:2 * H], W[:, 2 * H:]
    Uz, Ur, Uh = U[:, :H], U[:, H:2 * H], U[:, 2 * H:]
    bz, br, bh = b[:H], b[H:2 * H], b[2 * H:]
    h = torch.zeros((n, H), dtype=W.dtype)
    a_zs, a_rs = [], []
    for t in range(T):
        xt = x[:, t, :]
        xz, xr, xh = [xt if g is None else xt * g for g in m]
        a_z = xz @ Wz + bz + h @ Uz
        a_r = xr @ Wr + br + h @ Ur
        z = torch.clamp(0.2 * a_z + 0.5, 0.0, 1.0)
        r = torch.clamp(0.2 * a_r + 0.5, 0.0, 1.0)
        c = xh @ Wh + bh + (r * h) @ Uh
        h = z * h + (1.0 - z) * c
        a_zs.append(a_z)
        a_rs.append(a_r)
    logit = h @ wd + bd[0]
    return {'p': torch.sigmoid(logit), 'logit': logit, 'a_z': torch.stack(a_zs), 'a_r': torch.stack(a_rs)}


def weighted_log_loss(p, y, loss_bias):
    """functions.py:47-50, literally"""
    pos = (-y * torch.log(p + EPS)).mean()
    neg = (-(1.0 - y) * torch.log(1.0 - p + EPS)).mean()
    return loss_bias * neg + (1.0 - loss_bias) * pos


def loss_fn(params, x, y, masks=None, loss_bias=0.7):
    out = forward(params, x, masks)
    yt = torch.as_tensor(np.asarray(y, dtype=np.float64).reshape(-1), dtype=params[0].dtype)
    return weighted_log_loss(out['p'], yt, loss_bias), out


def loss_and_grads(weights, x, y, masks=None, loss_bias=0.7, dtype=torch.float64):
    """-> dict(loss, grads {name: array in the Keras shapes}, p [N], logit [N], a_z, a_r [T, N, H]) as float64 numpy"""
    params = tensors(weights, dtype)
    loss, out = loss_fn(params, x, y, masks, loss_bias)
    grads = torch.autograd.grad(loss, params)
    res = {k: v.detach().double().numpy() for k, v in out.items()}
    res['loss'] = float(loss.detach())
    res['grads'] = {name: g.double().numpy() for name, g in zip(NAMES, grads)}
    return res


def flat_grads(res) -> np.ndarray:
    """the gradients in the trainer's flat order"""
    return np.concatenate([res['grads'][n].reshape(-1) for n in NAMES])


def kink_safe(res, delta=1e-3, max_logit=8.0) -> np.ndarray:
    """bool [N]: every a_z, a_r of the sample at least ``delta`` from +-2.5 and |logit| <= max_logit"""
    a = np.concatenate([res['a_z'], res['a_r']], axis=2)                     # [T, N, 2H]
    far = (np.abs(np.abs(a) - 2.5) >= delta).all(axis=(0, 2))
    return far & (np.abs(res['logit']) <= max_logit)


def pick_kink_safe(weights, x, masks=None, delta=1e-3):
    """indices of the kink-safe candidates (the forward pass does not depend on the targets)"""
    params = tensors(weights, requires_grad=False)
    with torch.no_grad():
        out = {k: v.numpy() for k, v in forward(params, x, masks).items()}
    return np.flatnonzero(kink_safe(out, delta))


def rmsprop(theta, accum, g, lr=1e-3, rho=0.9, eps=1e-7):
    """keras.optimizers.RMSprop, in the dtype of the arguments"""
    accum = rho * accum + (1.0 - rho) * g * g
    return theta - lr * g / (np.sqrt(accum) + eps), accum


def mask_function(seed, step, n, feature_size, rate) -> np.ndarray:
    """numpy uint64 restatement of the documented mask function (include/precise_engine.h, pe_train_dropout_masks)"""
    M = np.uint64
    G = M(0x9E3779B97F4A7C15)

    def mix(v):
        v = v ^ (v >> M(30))
        v = v * M(0xBF58476D1CE4E5B9)
        v = v ^ (v >> M(27))
        v = v * M(0x94D049BB133111EB)
        return v ^ (v >> M(31))

    with np.errstate(over='ignore'):
        key = mix(mix(np.array([seed], dtype=M) + G) ^ (np.array([step], dtype=M) + G))
        gate = np.arange(3, dtype=M).reshape(3, 1, 1)
        pos = np.arange(n, dtype=M).reshape(1, n, 1)
        f = np.arange(feature_size, dtype=M).reshape(1, 1, feature_size)
        ctr = (pos << M(7)) | (gate << M(5)) | f
        bits = mix(key + G * (ctr + M(1)))
    u = (bits >> M(40)).astype(np.float32) * np.float32(2.0 ** -24)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
    return np.where(u >= np.float32(rate), scale, np.float32(0.0)).astype(np.float32)
