"""
Float64 reference for the training kernels.  TEST INFRASTRUCTURE ONLY.

The forward pass of ``oracle/keras_gru.py`` K1-K8 with the training-time input dropout of Keras 2.2.4 ``GRUCell``
(implementation 1: one mask per gate, the same for every timestep, multiplying x_t before that gate's input product), the
reference's ``weighted_log_loss`` (functions.py:47-50) and gradients by torch autograd, all in float64 on the CPU (``dtype``
may be lowered to float32 to measure the float32 floor).  It also returns every gate pre-activation and the logit, from which
the tests pick kink-safe samples: the hard sigmoid has kinks at pre-activation +-2.5, and a float32 kernel may legitimately
land on the other side of one.

Beyond |logit| of about 8 the float64 head is no reference for the kernel any more: the head is float32 by contract (DESIGN.md
4.9).  ``head32`` restates it in numpy float32, ``grads_from_ds`` is the float64 backward pass behind a given ds, and
``logit_bands`` names the regions of the logit the tests pick their samples from.
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


def forward_numpy(weights, x, masks=None, dtype=torch.float64):
    """``forward`` without a graph, as float64 numpy arrays (``dtype`` float32: the float32 floor of the forward pass)"""
    params = tensors(weights, dtype, requires_grad=False)
    with torch.no_grad():
        return {k: v.double().numpy() for k, v in forward(params, x, masks).items()}


def pick_kink_safe(weights, x, masks=None, delta=1e-3, max_logit=8.0):
    """indices of the kink-safe candidates (the forward pass does not depend on the targets)"""
    return np.flatnonzero(kink_safe(forward_numpy(weights, x, masks), delta, max_logit))


# ---- the float32 head ("The head is float32 by contract") -------------------------------------------------
BANDS = ('neg_sat', 'neg', 'mid', 'pos', 'edge', 'one')


def logit_bands(logit) -> np.ndarray:
    """[N] of BANDS: neg_sat (-inf, -19], neg (-19, -8], mid (-8, 8), pos [8, 17), edge [17, 19), one [19, inf).
    From 19 upward 1 - sigmoid <= 5.6e-9 < 2^-25, so the float32 sigmoid is 1.0f whatever the last bits of the logit;
    in ``edge`` it may be 1.0f or one or two ulps below."""
    logit = np.asarray(logit, dtype=np.float64)
    out = np.full(logit.shape, 'mid', dtype='<U7')
    out[logit <= -8.0] = 'neg'
    out[logit <= -19.0] = 'neg_sat'
    out[logit >= 8.0] = 'pos'
    out[logit >= 17.0] = 'edge'
    out[logit >= 19.0] = 'one'
    return out


def head32(p, y, loss_bias, n):
    """The head in float32, every operation rounded where the training kernel rounds it: p, y float32 (scalars or [N]),
    n the batch size the means divide by -> (ds, loss_neg, loss_pos) as float64.

        q = fl(fl(1 - p) + eps)                 pe = fl(p + eps)                           eps = fl32(1e-7)
        dp = fl(fl(fl(fl(b (1 - y)) / q) - fl(fl(fl(1 - b) y) / pe)) inv_n)              b = fl32(loss_bias), inv_n = fl(1 / n)
        ds = fl(fl(dp p) (1 - p))

    loss_neg = -(1 - y) log(q) and loss_pos = -y log(pe) per sample, the logarithms taken in float64 OF the float32 q and
    pe; the loss is b mean(loss_neg) + (1 - b) mean(loss_pos).  At p == 1.0f q is eps, dp is finite and ds is exactly +-0."""
    f = np.float32
    p, y = np.asarray(p, dtype=f), np.asarray(y, dtype=f)
    one, eps, beta = f(1.0), f(EPS), f(loss_bias)
    inv_n = one / f(n)
    q = (one - p) + eps
    pe = p + eps
    dp = ((beta * (one - y)) / q - ((one - beta) * y) / pe) * inv_n
    ds = (dp * p) * (one - p)
    assert all(v.dtype == f for v in (q, pe, dp, ds))
    y64 = y.astype(np.float64)
    return ds.astype(np.float64), -(1.0 - y64) * np.log(q.astype(np.float64)), -y64 * np.log(pe.astype(np.float64))


def head32_loss(p, y, loss_bias) -> float:
    """the loss of the batch from ``head32``'s per-sample terms, the means and the weighting in float64"""
    _, neg, pos = head32(p, y, loss_bias, len(np.atleast_1d(p)))
    beta = float(np.float32(loss_bias))
    return beta * float(np.mean(neg)) + (1.0 - beta) * float(np.mean(pos))


def grads_from_ds(weights, x, masks, ds, dtype=torch.float64):
    """The Jacobian of the logits contracted with a GIVEN ds [N] (autograd over ``forward``): what the backward pass owes
    once the head has spoken -> {name: array in the Keras shapes} as float64 numpy (``dtype`` float32: the float32 floor)"""
    params = tensors(weights, dtype)
    logit = forward(params, x, masks)['logit']
    seed = torch.as_tensor(np.asarray(ds, dtype=np.float64).reshape(-1), dtype=dtype)
    grads = torch.autograd.grad(logit, params, grad_outputs=seed)
    return {name: g.double().numpy() for name, g in zip(NAMES, grads)}


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
