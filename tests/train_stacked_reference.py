"""
Float64 reference for the stacked training kernels.  TEST INFRASTRUCTURE ONLY.

``train_reference.py`` for one OR two GRU layers: Sequential[GRU(H1, linear, dropout, return_sequences), GRU(H2, linear,
dropout), Dense(1, sigmoid)], every layer a Keras 2.2.4 ``GRUCell`` of implementation 1 (``reset_after=False``, gate order
z|r|h, hard sigmoid) with its own per-gate input masks, the same for every timestep: layer 0's multiply x_t, layer 1's
multiply h1_t, before that gate's input product.  Loss, gradients by torch autograd, float64 on the CPU (``dtype`` may be
lowered to float32 to measure the float32 floor).  ``head32`` and ``rmsprop`` are train_reference's.
"""
import numpy as np
import torch

from train_reference import EPS, head32, rmsprop, weighted_log_loss        # noqa: F401

LAYER_NAMES = ('kernel', 'recurrent_kernel', 'bias')


def names(n_layers):
    """the flat order: per layer kernel_l | recurrent_kernel_l | bias_l, then dense_kernel | dense_bias"""
    return tuple('%s_%d' % (n, l) for l in range(n_layers) for n in LAYER_NAMES) + ('dense_kernel', 'dense_bias')


def tensors(weights, dtype=torch.float64, requires_grad=True):
    src = [a for layer in weights['gru'] for a in layer]
    src += [np.asarray(weights['dense_kernel']).reshape(-1), np.asarray(weights['dense_bias']).reshape(-1)]
    return [torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype, requires_grad=requires_grad) for a in src]


def _masks_per_layer(masks, n_layers):
    """None, one [3, N, F] array (one layer) or a sequence of one per layer (entries may be None)"""
    if masks is None:
        return [None] * n_layers
    if isinstance(masks, (tuple, list)):
        assert len(masks) == n_layers
        return list(masks)
    assert n_layers == 1
    return [masks]


def gru_layer(x, W, U, b, masks):
    """x [N, T, K] -> (h sequence [N, T, H], a_z, a_r [T, N, H])"""
    H = U.shape[0]
    n, T, _ = x.shape
    m = [None] * 3 if masks is None else [torch.as_tensor(np.asarray(g, dtype=np.float64), dtype=W.dtype) for g in masks]
    Wz, Wr, Wh = W[:, :H], W[:, H:2 * H], W[:, 2 * H:]
    Uz, Ur, Uh = U[:, :H], U[:, H:2 * H], U[:, 2 * H:]
    bz, br, bh = b[:H], b[H:2 * H], b[2 * H:]
    h = torch.zeros((n, H), dtype=W.dtype)
    hs, a_zs, a_rs = [], [], []
    for t in range(T):
        xt = x[:, t, :]
        xz, xr, xh = [xt if g is None else xt * g for g in m]
        a_z = xz @ Wz + bz + h @ Uz
        a_r = xr @ Wr + br + h @ Ur
        z = torch.clamp(0.2 * a_z + 0.5, 0.0, 1.0)
        r = torch.clamp(0.2 * a_r + 0.5, 0.0, 1.0)
        c = xh @ Wh + bh + (r * h) @ Uh
        h = z * h + (1.0 - z) * c
        hs.append(h)
        a_zs.append(a_z)
        a_rs.append(a_r)
    return torch.stack(hs, dim=1), torch.stack(a_zs), torch.stack(a_rs)


def forward(params, x, masks=None):
    """x [N, T, F], masks per layer -> dict(p [N], logit [N], a_z / a_r: one [T, N, H_l] per layer)"""
    n_layers = (len(params) - 2) // 3
    seq = torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=params[0].dtype)
    a_z, a_r = [], []
    for l, m in enumerate(_masks_per_layer(masks, n_layers)):
        seq, az, ar = gru_layer(seq, *params[3 * l:3 * l + 3], m)
        a_z.append(az)
        a_r.append(ar)
    logit = seq[:, -1, :] @ params[-2] + params[-1][0]
    return {'p': torch.sigmoid(logit), 'logit': logit, 'a_z': a_z, 'a_r': a_r}


def _numpy(out):
    return {k: [a.detach().double().numpy() for a in v] if isinstance(v, list) else v.detach().double().numpy() for k, v in out.items()}


def loss_and_grads(weights, x, y, masks=None, loss_bias=0.7, dtype=torch.float64):
    """-> dict(loss, grads {name: array in the Keras shapes}, p, logit, a_z, a_r) as float64 numpy"""
    params = tensors(weights, dtype)
    out = forward(params, x, masks)
    yt = torch.as_tensor(np.asarray(y, dtype=np.float64).reshape(-1), dtype=dtype)
    loss = weighted_log_loss(out['p'], yt, loss_bias)
    grads = torch.autograd.grad(loss, params)
    res = _numpy(out)
    res['loss'] = float(loss.detach())
    res['grads'] = {name: g.double().numpy() for name, g in zip(names(len(weights['gru'])), grads)}
    return res


def flat_grads(res) -> np.ndarray:
    """the gradients in the trainer's flat order"""
    return np.concatenate([g.reshape(-1) for g in res['grads'].values()])


def forward_numpy(weights, x, masks=None, dtype=torch.float64):
    params = tensors(weights, dtype, requires_grad=False)
    with torch.no_grad():
        return _numpy(forward(params, x, masks))


def kink_safe(res, delta=1e-3, max_logit=8.0) -> np.ndarray:
    """bool [N]: every a_z, a_r of every layer at least ``delta`` from +-2.5 and |logit| <= max_logit"""
    a = np.concatenate(list(res['a_z']) + list(res['a_r']), axis=2)
    far = (np.abs(np.abs(a) - 2.5) >= delta).all(axis=(0, 2))
    return far & (np.abs(res['logit']) <= max_logit)


def saturation(res, layer) -> float:
    """share of the layer's gate values (z and r, every step and unit) on the flat part of the hard sigmoid"""
    a = np.abs(np.concatenate([res['a_z'][layer], res['a_r'][layer]], axis=2))
    return float((a > 2.5).mean())


def grads_from_ds(weights, x, masks, ds, dtype=torch.float64):
    """the Jacobian of the logits contracted with a GIVEN ds [N] -> {name: array} as float64 numpy"""
    params = tensors(weights, dtype)
    logit = forward(params, x, masks)['logit']
    seed = torch.as_tensor(np.asarray(ds, dtype=np.float64).reshape(-1), dtype=dtype)
    grads = torch.autograd.grad(logit, params, grad_outputs=seed)
    return {name: g.double().numpy() for name, g in zip(names(len(weights['gru'])), grads)}


def mask_function(seed, step, n, width, rate, layer=0) -> np.ndarray:
    """numpy uint64 restatement of the documented mask function (include/precise_engine.h, pe_train_dropout_masks_layer):
    float32 [3, n, width]"""
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
        f = np.arange(width, dtype=M).reshape(1, 1, width)
        if layer == 0:
            ctr = (pos << M(7)) | (gate << M(5)) | f
        else:
            key = mix(key ^ G)
            ctr = (pos << M(10)) | (gate << M(8)) | f
        bits = mix(key + G * (ctr + M(1)))
    u = (bits >> M(40)).astype(np.float32) * np.float32(2.0 ** -24)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
    return np.where(u >= np.float32(rate), scale, np.float32(0.0)).astype(np.float32)
