"""
CPU restatement of the arithmetic CONTRACT of the bf16-operand network (``gru_precision='bf16'``), as the comments at the
top of ``mycroft_precise_amd/csrc/gru_bf16_device.h`` and ``gru_b20_device.h`` and the packers in ``csrc/engine.hip``
(``to_bf16``, ``pack_gru_weights_bf16``, ``pack_gru_weights_b20``) state it.  TEST INFRASTRUCTURE ONLY: nothing under
``mycroft_precise_amd/`` imports it.

The network is the one of ``keras_gru.py`` (K1-K7, one GRU layer + Dense(1) + sigmoid).  What differs is WHERE values are
rounded to bfloat16 (8 significant bits, round to nearest even):

  B1  kernel W and recurrent kernel U: every entry rounded once, on the host.
  B2  bias b: the pair  hi = bf16(b),  lo = bf16(b - hi)  rides in the input contraction against 1.0; hi + lo is what
      the gates see (residual <= 2^-17 |b|).
  B3  the feature row x_t: rounded as it becomes an MFMA operand.
  B4  use_delta, rows='f32' (float32 ring rows, row sequences): d_t = float32(x_t) - float32(x_(t-1)) formed in float32
      from the UNROUNDED rows (zero at t = 0), then rounded.  An explicit batch carries its delta columns: they are
      features like any other (pass them in ``x`` with ``use_delta=False``) and are only rounded.
  B5  use_delta, rows='bf16' (ring_precision='bf16'): the ring holds rounded rows, so d_t is formed, in float32, from the
      ROUNDED rows, then rounded.  B4 and B5 give different operands.
  B6  the hidden state h (operand of the z and r gates) and r*h (operand of the candidate): rounded as operands.  The
      state that is carried, blended and fed to the Dense head is NOT rounded.
  B7  everything else is wide: accumulation, gates hs(v) = clip(0.2 v + 0.5, 0, 1), h' = z h + (1 - z) c, the Dense
      weights and bias (unrounded), the sigmoid.

"Wide" is float32 on the device and its summation order is the MFMA's.  ``variant`` picks one faithful evaluation:

  'f64'       accumulate, gates and state in float64: THE reference the kernels are compared with
  'f32'       float32 gates, state and head; float64 dot products rounded once
  'f32_fwd'   float32 accumulation term by term, k ascending (input terms, bias hi, lo, then recurrent terms)
  'f32_rev'   the same chain with every group in descending k

The variants exist to measure how far faithful evaluations of the same contract lie apart.  Almost always that is a
few float32 ulps of the output; now and then a state value sits so close to a bf16 rounding boundary that two variants
round it to different operands (a "flip"), and from there on they are a bf16 ulp apart.  ``trace=True`` returns a
digest of every operand bit pattern per window, so such windows can be told from the others.
"""
import hashlib

import numpy as np

VARIANTS = ('f64', 'f32', 'f32_fwd', 'f32_rev')


def _quantum(v):
    """spacing of bfloat16 at the magnitude of v (float64, finite): 2^(e - 7) for 2^e <= |v| < 2^(e + 1)"""
    _, e = np.frexp(v)
    return np.ldexp(1.0, np.maximum(e, -125) - 8)          # (below 2^-126: the denormal spacing 2^-133)


def round_bf16(v, mode='rne'):
    """float array -> float64 array of bfloat16 values.  mode: 'rne' round to nearest even (the contract), 'trunc' toward
    zero and 'none' the identity (both only for fault injection and for the tie with keras_gru)."""
    v = np.asarray(v, dtype=np.float64)
    if mode == 'none':
        return v
    fin = np.isfinite(v)
    s = np.where(fin, v, 0.0)
    q = _quantum(s)
    r = (np.rint(s / q) if mode == 'rne' else np.trunc(s / q)) * q       # s / q is exact; rint rounds halves to even
    r = np.where(np.abs(r) >= 2.0 ** 128, np.copysign(np.inf, s), r)
    return np.where(fin, r, v)


def bf16_bits(v):
    """bit patterns (uint16) of values that are exactly representable in bfloat16"""
    return (np.asarray(v, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def split_bias(b, mode='rne'):
    """B2 -> (hi, lo), float64"""
    b = np.asarray(b, dtype=np.float32)
    hi = round_bf16(b, mode)
    lo = round_bf16((b - hi.astype(np.float32)).astype(np.float32), mode)     # (the float32 difference is exact)
    return hi, lo


def _operands(x, n_in, use_delta, rows, mode):
    """B3-B5: float32 rows [n, T, F] -> rounded input operands [n, T, n_in] (float64 holding bf16 values)"""
    x = np.asarray(x, dtype=np.float32)
    if not use_delta:
        if x.shape[2] != n_in:
            raise ValueError('the layer takes %d inputs, x has %d columns' % (n_in, x.shape[2]))
        return round_bf16(x, mode)
    if 2 * x.shape[2] != n_in:
        raise ValueError('use_delta: the layer takes %d inputs, x must have %d columns' % (n_in, n_in // 2))
    if rows == 'f32':
        src = x
    elif rows == 'bf16':
        src = round_bf16(x, mode).astype(np.float32)
    else:
        raise ValueError("rows must be 'f32' or 'bf16'")
    d = np.zeros_like(src)
    with np.errstate(invalid='ignore', over='ignore'):
        d[:, 1:] = src[:, 1:] - src[:, :-1]                                    # float32 arithmetic
    return np.concatenate([round_bf16(x, mode), round_bf16(d, mode)], axis=2)


def _affine(variant, xb, W, hi, lo, hb, U):
    """x . W + (hi + lo) + h . U over the given columns, in the variant's arithmetic"""
    with np.errstate(invalid='ignore', over='ignore'):
        if variant in ('f64', 'f32'):
            a = xb @ W + (hi + lo) + hb @ U
            return a if variant == 'f64' else a.astype(np.float32)
        f = np.float32
        px = (xb[:, :, None] * W[None]).astype(f)            # products of two bf16 values: exact in float32
        ph = (hb[:, :, None] * U[None]).astype(f)
        a = np.zeros((xb.shape[0], W.shape[1]), dtype=f)
        if variant == 'f32_fwd':
            for k in range(px.shape[1]):
                a = a + px[:, k]
            a = a + hi.astype(f)
            a = a + lo.astype(f)
            for k in range(ph.shape[1]):
                a = a + ph[:, k]
        else:
            a = a + lo.astype(f)
            a = a + hi.astype(f)
            for k in range(px.shape[1] - 1, -1, -1):
                a = a + px[:, k]
            for k in range(ph.shape[1] - 1, -1, -1):
                a = a + ph[:, k]
        return a


def predict(x, weights, *, use_delta=False, rows='f32', variant='f64', trace=False,
            rounding='rne', round_h=True, bias_lo=True, bump=None):
    """
    x: [n, T, F] feature rows (read as float32, what the kernels load); with ``use_delta`` the layer has 2 F inputs and
    the first differences are formed here (B4 / B5), otherwise x holds every input column of the layer.
    weights: as ``keras_gru.predict`` takes them, ONE GRU layer.
    -> float64 probabilities [n]; with ``trace`` also a list of n digests (hex) of every bf16 operand (x, h, r*h) of
    every timestep.

    For fault injection and measurement only: ``rounding`` ('rne' | 'trunc' | 'none') replaces the rounding of every
    B1-B6 value, ``round_h=False`` leaves h and r*h unrounded, ``bias_lo=False`` drops the lo half of the bias,
    ``bump=(t, unit, sign)`` moves the rounded h operand of one unit at one timestep by one bf16 ulp.
    """
    if variant not in VARIANTS:
        raise ValueError('variant must be one of %r' % (VARIANTS,))
    if len(weights['gru']) != 1:
        raise ValueError('the bf16 network is one GRU layer')
    kernel, rec, bias = weights['gru'][0]
    H = rec.shape[0]
    W = round_bf16(np.asarray(kernel, dtype=np.float32), rounding)           # B1
    U = round_bf16(np.asarray(rec, dtype=np.float32), rounding)
    if rounding == 'none':
        hi, lo = np.asarray(bias, dtype=np.float64), np.zeros(3 * H)
    else:
        hi, lo = split_bias(bias, rounding)                                   # B2
    if not bias_lo:
        lo = np.zeros_like(lo)
    xb = _operands(x, W.shape[0], use_delta, rows, rounding)                 # B3-B5
    n, T, _ = xb.shape
    dt = np.float64 if variant == 'f64' else np.float32
    hmode = rounding if round_h else 'none'
    h = np.zeros((n, H), dtype=dt)
    ops = []
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(T):
            hb = round_bf16(h, hmode)                                         # B6
            if bump is not None and bump[0] == t:
                hb = hb.copy()
                hb[:, bump[1]] += bump[2] * _quantum(np.where(np.isfinite(hb[:, bump[1]]), hb[:, bump[1]], 0.0))
            a = _affine(variant, xb[:, t], W[:, :2 * H], hi[:2 * H], lo[:2 * H], hb, U[:, :2 * H])
            g = np.clip(dt(0.2) * a + dt(0.5), dt(0.0), dt(1.0))
            z, r = g[:, :H], g[:, H:]
            rh = r * h
            rhb = round_bf16(rh, hmode)                                       # B6
            c = _affine(variant, xb[:, t], W[:, 2 * H:], hi[2 * H:], lo[2 * H:], rhb, U[:, 2 * H:])
            h = z * h + (dt(1.0) - z) * c                                     # B7
            if trace:
                ops += [bf16_bits(xb[:, t]), bf16_bits(round_bf16(hb)), bf16_bits(round_bf16(rhb))]
        wd = np.asarray(weights['dense_kernel'], dtype=dt).reshape(-1)
        bd = dt(np.asarray(weights['dense_bias'], dtype=np.float32).reshape(-1)[0])
        p = (dt(1.0) / (dt(1.0) + np.exp(-(h @ wd + bd)))).astype(np.float64)
    if not trace:
        return p
    allops = np.ascontiguousarray(np.concatenate(ops, axis=1))
    return p, [hashlib.sha1(row.tobytes()).hexdigest() for row in allops]


def flip_free(x, weights, **kw):
    """-> (mask [n]: all four variants round every operand of the window alike, {variant: probabilities})"""
    out, dig = {}, {}
    for v in VARIANTS:
        out[v], dig[v] = predict(x, weights, variant=v, trace=True, **kw)
    mask = np.array([len({dig[v][i] for v in VARIANTS}) == 1 for i in range(len(out['f64']))], dtype=bool)
    return mask, out


def spread(outs, mask):
    """largest distance between two variants on the windows of ``mask``"""
    p = np.stack([outs[v] for v in VARIANTS])
    if not mask.any():
        return 0.0
    return float((p.max(axis=0) - p.min(axis=0))[mask].max())


def one_ulp_effect(x, weights, *, n_pairs=8, seed=0, **kw):
    """The largest change of the output, over the windows of x, when ONE h operand at ONE timestep moves by one bf16
    ulp (either way): what a single flip costs.  (timestep, unit) pairs: t = 0, t = T - 1 and seeded random others."""
    kernel, rec, _ = weights['gru'][0]
    H, T = rec.shape[0], np.asarray(x).shape[1]
    rng = np.random.default_rng(seed)
    pairs = [(0, int(rng.integers(H))), (T - 1, int(rng.integers(H)))]
    while len(pairs) < max(5, n_pairs):
        pairs.append((int(rng.integers(1, max(T - 1, 2))) % T, int(rng.integers(H))))
    base = predict(x, weights, variant='f64', **kw)
    worst = 0.0
    for t, u in pairs:
        for sign in (1.0, -1.0):
            d = np.abs(predict(x, weights, variant='f64', bump=(t, u, sign), **kw) - base)
            d = d[np.isfinite(d)]
            if d.size:
                worst = max(worst, float(d.max()))
    return worst
