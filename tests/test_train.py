"""GPU: the training kernels (csrc/gru_train_device.h) against the float64 autograd reference of train_reference.py.

Bounds: gradients per tensor max|d| / max|reference tensor| <= 1e-5 (about 20x the float32 floor, which is
torch float32 autograd against the same float64 reference: 0.4e-7 .. 5.4e-7), loss <= 1e-6, probabilities <= 1e-5.  All
batches are built from kink-safe candidates only (train_reference.kink_safe): every hard-sigmoid pre-activation at least
1e-3 from +-2.5 and |logit| <= 8 in the float64 reference, and every test asserts that at least half its candidates pass.

The saturated-head tests drop the logit limit (the gate-kink rule stays) and hold the kernel to the float32 head contract
(train_reference.head32, DESIGN.md 4.9 "The head is float32 by contract"): beyond logit 12 a float64 head is no reference for
ds.  Their bounds follow the same 20x rule, the floors measured on the CPU by saturated_floors() below with torch float32 in
the kernel's place, over the ten cases of test_gradients_saturated_head:
  probabilities in neg and neg_sat, relative to float64: floor 1.78e-5 (2.41e-5 with masks), bound 20 x 2.41e-5 = 4.8e-4;
    in mid PROB_TOL as everywhere; in pos and one |p - sigmoid64| <= 2^-23 (two float32 roundings at 2^-24 each), in one p == 1.0f;
  gradients, the float64 Jacobian contracted with head32 of the kernel's own probabilities: floor 1.34e-6 (2.43e-6 with
    masks), and 20x that is above GRAD_TOL = 1e-5, so the bounds are 20 x 1.34e-6 = 2.7e-5 and 20 x 2.43e-6 = 4.9e-5 with masks;
  loss, relative to head32's loss: floor 9.81e-8, bound 20 x 9.81e-8 = 1.96e-6 (LOSS_TOL = 1e-6 absolute is less than the
    float32 spacing of a loss near 5).
"""
import functools

import numpy as np
import pytest

import train_reference as ref
from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.model import ModelParams, load_weights
from mycroft_precise_amd.params import pr

pytestmark = pytest.mark.gpu

GRAD_TOL, LOSS_TOL, PROB_TOL = 1e-5, 1e-6, 1e-5
SAT_PROB_REL_TOL, SAT_GRAD_TOL, SAT_GRAD_TOL_MASKS, SAT_LOSS_REL_TOL = 20 * 2.41e-5, 20 * 1.34e-6, 20 * 2.43e-6, 20 * 9.81e-8


@functools.lru_cache(maxsize=None)
def mfcc_windows(n):
    """n real MFCC windows [29, 13] of synth.stream_pcm (the oracle's vectorizer; eight streams, a window every 3 frames)"""
    from oracle import listener
    p = listener.Params()
    per = -(-n // 8)
    frames = p.n_features + 3 * (per - 1)
    out = []
    for s in range(8):
        pcm = synth.stream_pcm(s, p.window_samples + p.hop_samples * (frames - 1))
        f = listener.vectorize_raw(pcm.astype(np.float32) / np.float32(32768.0), p)
        out += [f[3 * i:3 * i + p.n_features] for i in range(per)]
    return np.asarray(out[:n], dtype=np.float32)


def candidates(family, n, T=29, F=13, seed=0):
    rng = np.random.default_rng(seed)
    if family == 'mfcc':
        assert (T, F) == (29, 13)
        return mfcc_windows(n)
    return rng.normal(0.0, 3.0 if family == 'n03' else 1.0, (n, T, F)).astype(np.float32)


def safe_batch(weights, family, n, n_candidates, T=29, F=13, rate=0.0, seed=0):
    """-> (x [n, T, F] float32, masks [3, n, F] or None): the first n kink-safe candidates"""
    x = candidates(family, n_candidates, T, F, seed)
    masks = _lib.dropout_masks(seed, 1, n_candidates, F, rate) if rate > 0 else None
    keep = ref.pick_kink_safe(weights, x, masks)
    print('%s: %d of %d candidates kink-safe' % (family, keep.size, n_candidates))
    assert keep.size >= n_candidates / 2 and keep.size >= n
    keep = keep[:n]
    return x[keep], (masks[:, keep] if masks is not None else None)


def targets_for(n, seed=0):
    return (np.random.default_rng(100 + seed).random(n) < 0.5).astype(np.float32)


def check_against_reference(weights, x, y, masks=None, loss_bias=0.7, T=29):
    F, H = weights['gru'][0][0].shape[0], weights['gru'][0][1].shape[0]
    want = ref.loss_and_grads(weights, x, y, masks, loss_bias)
    t = _lib.HipTrainer(weights, T, F)
    try:
        loss, grads, probs = t.loss_grad(x, y, masks=masks, loss_bias=loss_bias)
        loss2, grads2, probs2 = t.loss_grad(x, y, masks=masks, loss_bias=loss_bias)
    finally:
        t.close()
    assert loss == loss2 and np.array_equal(grads.view(np.uint32), grads2.view(np.uint32)) and np.array_equal(probs, probs2)
    sizes = np.cumsum([F * 3 * H, H * 3 * H, 3 * H, H])
    worst = {}
    for name, g in zip(ref.NAMES, np.split(grads.astype(np.float64), sizes)):
        w = want['grads'][name].reshape(-1)
        scale = float(np.abs(w).max())
        worst[name] = float(np.abs(g - w).max()) / scale if scale > 0 else float(np.abs(g).max())
    d_loss = abs(loss - want['loss'])
    d_prob = float(np.abs(probs - want['p']).max())
    print('N=%d T=%d F=%d H=%d bias=%g: grads %s loss %.3g probs %.3g' %
          (len(x), T, F, H, loss_bias, ' '.join('%s %.3g' % kv for kv in worst.items()), d_loss, d_prob))
    assert max(worst.values()) <= GRAD_TOL, worst
    assert d_loss <= LOSS_TOL
    assert d_prob <= PROB_TOL
    return worst


@pytest.mark.parametrize('n', [1, 15, 16, 17, 33, 240])
def test_gradients_tile_edges(stock_weights, n):
    x, _ = safe_batch(stock_weights, 'n03', n, 480, seed=n)
    check_against_reference(stock_weights, x, targets_for(n, n))


@pytest.mark.parametrize('rate', [0.0, 0.2])
@pytest.mark.parametrize('family', ['n01', 'n03', 'mfcc'])
def test_gradients_input_families_and_supplied_masks(stock_weights, family, rate):
    x, masks = safe_batch(stock_weights, family, 120, 256, rate=rate, seed=7)
    check_against_reference(stock_weights, x, targets_for(120, 7), masks)


def test_gradients_more_tiles_than_compute_units(stock_weights):
    x, _ = safe_batch(stock_weights, 'n01', 5000, 5600, seed=11)
    check_against_reference(stock_weights, x, targets_for(5000, 11))


@pytest.mark.parametrize('T,F,H', [(1, 13, 20), (2, 13, 20), (29, 26, 20), (29, 1, 1), (29, 13, 32), (64, 32, 32)])
def test_gradients_shapes(stock_weights, T, F, H):
    weights = stock_weights if (F, H) == (13, 20) else synth.make_weights(F, (H,))
    x, masks = safe_batch(weights, 'n01', 33, 256, T=T, F=F, rate=0.2, seed=T + F + H)
    check_against_reference(weights, x, targets_for(33, T), masks, T=T)


@pytest.mark.parametrize('target', [0.0, 1.0])
def test_gradients_constant_targets(stock_weights, target):
    x, masks = safe_batch(stock_weights, 'n03', 33, 256, rate=0.2, seed=3)
    check_against_reference(stock_weights, x, np.full(33, target, dtype=np.float32), masks)


@pytest.mark.parametrize('loss_bias', [0.7, 0.0, 1.0])
def test_gradients_loss_bias(stock_weights, loss_bias):
    x, _ = safe_batch(stock_weights, 'mfcc', 33, 256, seed=5)
    check_against_reference(stock_weights, x, targets_for(33, 5), loss_bias=loss_bias)


@pytest.mark.parametrize('F', [1, 13, 32])
@pytest.mark.parametrize('H', [2, 3, 5, 7, 8, 12, 21, 31])
def test_gradients_every_thread_layout(H, F):
    """Widths whose blocks have idle lanes (16 H no multiple of 64), an odd 3 H, the most gradient elements per thread
    (F = 32 at a small H) and one wave short of full (H = 31): one full tile and a tile of one sample."""
    weights = synth.make_weights(F, (H,))
    x, masks = safe_batch(weights, 'n01', 17, 256, T=3, F=F, rate=0.2, seed=H + F)
    check_against_reference(weights, x, targets_for(17, H), masks, T=3)


# ---- the saturated head ("The head is float32 by contract") -----------------------------------------------
def scaled_head(weights, factor=8.0):
    """the same GRU under a dense layer ``factor`` times as large (rounded to float32): logits out to +-50 and beyond"""
    f = np.float32(factor)
    return dict(weights, dense_kernel=(np.asarray(weights['dense_kernel'], dtype=np.float32) * f).astype(np.float32),
                dense_bias=(np.asarray(weights['dense_bias'], dtype=np.float32) * f).astype(np.float32))


SAT_N, SAT_CANDIDATES = 240, 480
_saturated = {}


def saturated_pool(stock_weights, rate=0.0):
    """480 'n03' candidates (seed 0) through the scaled stock network in float64, computed once per mask rate and left alone:
    dict(weights, x, masks, p, logit, bands, safe).  Kink-safe here keeps the gate-kink rule and drops the logit limit."""
    if rate not in _saturated:
        weights = scaled_head(stock_weights)
        x = candidates('n03', SAT_CANDIDATES, seed=0)
        masks = _lib.dropout_masks(0, 1, SAT_CANDIDATES, 13, rate) if rate > 0 else None
        out = ref.forward_numpy(weights, x, masks)
        safe = ref.kink_safe(out, max_logit=np.inf)
        bands = ref.logit_bands(out['logit'])
        print('rate %g: %d of %d candidates kink-safe, bands %s' %
              (rate, safe.sum(), SAT_CANDIDATES, {b: int((bands == b).sum()) for b in ref.BANDS}))
        _saturated[rate] = dict(weights=weights, x=x, masks=masks, p=out['p'], logit=out['logit'], bands=bands, safe=safe)
    return _saturated[rate]


def saturated_batch(stock_weights, n, bands, rate=0.0):
    """-> dict(weights, x [n], masks or None, p, bands, rows): the first n kink-safe candidates whose float64 logit lies in
    one of ``bands``; at least half the candidates are kink-safe and every band holds at least 16 of the n"""
    pool = saturated_pool(stock_weights, rate)
    assert pool['safe'].sum() >= SAT_CANDIDATES / 2
    rows = np.flatnonzero(pool['safe'] & np.isin(pool['bands'], bands))[:n]
    assert rows.size == n
    counts = {b: int((pool['bands'][rows] == b).sum()) for b in bands}
    print('%d kink-safe samples: %s' % (n, counts))
    assert min(counts.values()) >= 16, counts
    return dict(weights=pool['weights'], x=pool['x'][rows], masks=None if pool['masks'] is None else pool['masks'][:, rows],
                p=pool['p'][rows], bands=pool['bands'][rows], rows=rows)


ALL_BUT_EDGE = ('neg_sat', 'neg', 'mid', 'pos', 'one')


def saturated_targets(kind, n):
    return {'random': targets_for(n, 31), 'zeros': np.zeros(n, dtype=np.float32), 'ones': np.ones(n, dtype=np.float32)}[kind]


def rel_err(got, want):
    """|got - want| / |want|; a reference of exactly 0 asks for exactly 0"""
    return abs(got - want) / abs(want) if want != 0 else (0.0 if got == 0 else float('inf'))


def check_probabilities_in_bands(probs, want_p, bands):
    d = np.abs(probs.astype(np.float64) - want_p)
    mid, one = bands == 'mid', bands == 'one'
    high, low = (bands == 'pos') | one, (bands == 'neg') | (bands == 'neg_sat')
    assert not (bands == 'edge').any() and probs.dtype == np.float32
    figures = (float(d[mid].max()), float(d[high].max()), float((d[low] / want_p[low]).max()))
    print('probabilities: mid %.3g, pos and one %.3g (2^-23 = %.3g), neg and neg_sat relative %.3g' %
          (figures[0], figures[1], 2.0 ** -23, figures[2]))
    assert figures[0] <= PROB_TOL
    assert figures[1] <= 2.0 ** -23
    assert np.all(probs[one] == np.float32(1.0))
    assert figures[2] <= SAT_PROB_REL_TOL


def check_saturated(batch, y, loss_bias):
    """one loss_grad call: the probabilities against float64 band by band, then gradients and loss against the float32 head
    contract fed with the probabilities the kernel reported"""
    weights, x, masks, n = batch['weights'], batch['x'], batch['masks'], len(batch['x'])
    t = _lib.HipTrainer(weights, 29, 13)
    try:
        loss, grads, probs = t.loss_grad(x, y, masks=masks, loss_bias=loss_bias)
    finally:
        t.close()
    check_probabilities_in_bands(probs, batch['p'], batch['bands'])
    ds, _, _ = ref.head32(probs, y, loss_bias, n)
    want = ref.grads_from_ds(weights, x, masks, ds)
    worst = {}
    for name, g in zip(ref.NAMES, np.split(grads.astype(np.float64), np.cumsum([13 * 60, 20 * 60, 60, 20]))):
        w = want[name].reshape(-1)
        scale = float(np.abs(w).max())
        worst[name] = float(np.abs(g - w).max()) / scale if scale > 0 else (0.0 if not g.any() else float('inf'))
    want_loss = ref.head32_loss(probs, y, loss_bias)
    d_loss = rel_err(loss, want_loss)
    tol = SAT_GRAD_TOL_MASKS if masks is not None else SAT_GRAD_TOL
    print('bias %g, %d of %d targets 1: grads %s (bound %.3g) loss %.7g, relative %.3g' %
          (loss_bias, int(y.sum()), n, ' '.join('%s %.3g' % kv for kv in worst.items()), tol, loss, d_loss))
    assert np.all(np.isfinite(grads))
    assert max(worst.values()) <= tol, worst
    assert d_loss <= SAT_LOSS_REL_TOL
    return loss, grads, probs


SAT_CASES = [(targets, loss_bias, 0.0) for targets in ('random', 'zeros', 'ones') for loss_bias in (0.7, 0.0, 1.0)] + \
    [('random', 0.7, 0.2)]                                                       # (the last one with supplied masks)


@pytest.mark.parametrize('targets,loss_bias,rate', SAT_CASES)
def test_gradients_saturated_head(stock_weights, targets, loss_bias, rate):
    batch = saturated_batch(stock_weights, SAT_N, ALL_BUT_EDGE, rate)
    check_saturated(batch, saturated_targets(targets, SAT_N), loss_bias)


def test_head_is_the_float32_contract_bit_for_bit(stock_weights):
    """A batch of ONE sample under a dense kernel of zeros: the logit is dense_bias, and the gradient of dense_bias is
    0 + 1.0f ds (then fifteen times + 1.0f 0 for the empty places of the tile), which no rounding touches.  So it shows the
    kernel's ds itself, and that is head32 of the reported probability to the bit.  The sweeps cross the logits where 1 - p
    (11 .. 18, to p == 1.0f) or p (-17.5 .. -14.5) is within a few binades of eps: there a q or pe formed in another order
    is off by whole ulps, and one formed in another precision rounds to the neighbouring float32 on about one point in ten."""
    weights = dict(stock_weights, dense_kernel=np.zeros((20, 1), dtype=np.float32), dense_bias=np.zeros(1, dtype=np.float32))
    x = candidates('n01', 1, seed=9)
    t = _lib.HipTrainer(weights, 29, 13)
    theta = t.get_weights()
    seen = set()
    try:
        for lo, hi, n in ((-17.5, -14.5, 256), (11.0, 18.0, 128), (-8.0, 8.0, 16)):
            for logit in np.linspace(lo, hi, n).astype(np.float32):
                theta[-1] = logit
                t.set_weights(theta)
                for y in (0.0, 1.0):
                    target = np.array([y], dtype=np.float32)
                    _, grads, probs = t.loss_grad(x, target, loss_bias=0.7)
                    ds = np.float32(ref.head32(probs, target, 0.7, 1)[0][0])              # (a float32 widened: exact)
                    # (the logit is exact here; expf to a few ulps and two roundings: 2^-23 absolute or 1e-6 relative)
                    assert abs(float(probs[0]) - 1.0 / (1.0 + np.exp(-float(logit)))) <= max(2.0 ** -23, 1e-6 * float(probs[0]))
                    same = grads[-1] == 0 if ds == 0 else np.float32(grads[-1]).view(np.uint32) == ds.view(np.uint32)
                    assert same, (float(logit), y, float(probs[0]), float(grads[-1]), float(ds))
                    assert not grads[:-21].any()                 # delta_T = ds w_d = 0: nothing reaches the GRU
                seen.add(float(probs[0]))
    finally:
        t.close()
    assert 1.0 in seen and len(seen) >= 256                             # (p == 1.0f reached; the sweeps did not collapse)


def test_certain_and_wrong_batch_has_zero_gradient(stock_weights):
    """p == 1.0f: ds is exactly +-0 whatever the target (float32 Keras alike), so the batch teaches nothing -- by contract"""
    n, beta, rho = 33, 0.7, 0.9
    batch = saturated_batch(stock_weights, n, ('one',))
    x, y = batch['x'], targets_for(n, 41)
    assert 8 <= y.sum() <= n - 8
    other = saturated_batch(stock_weights, n, ('mid',))
    t = _lib.HipTrainer(batch['weights'], 29, 13)
    try:
        loss, grads, probs = t.loss_grad(x, y, loss_bias=beta)
        assert np.all(probs == np.float32(1.0))
        assert np.array_equal(grads, np.zeros_like(grads))                      # every entry +0.0 or -0.0, none NaN
        eps32 = float(np.float32(ref.EPS))
        _, _, pos_term = ref.head32(np.ones(n, dtype=np.float32), y, beta, n)
        b = float(np.float32(beta))
        want_loss = b * float(np.mean(1.0 - y)) * -np.log(eps32) + (1.0 - b) * float(np.mean(pos_term))
        print('loss %.7g, expected %.7g: relative %.3g' % (loss, want_loss, rel_err(loss, want_loss)))
        assert rel_err(loss, want_loss) <= SAT_LOSS_REL_TOL
        # a step on that batch moves nothing
        theta = t.get_weights()
        t.set_data(np.concatenate([x, other['x']]), np.concatenate([y, targets_for(n, 42)]))
        certain, ordinary = np.arange(n, dtype=np.int32), np.arange(n, 2 * n, dtype=np.int32)
        step_loss = t.step(certain, 0.0, 0, 0, beta, 1e-3, rho, 1e-7, 0)
        assert np.float32(step_loss) == np.float32(loss)
        assert np.array_equal(t.get_weights().view(np.uint32), theta.view(np.uint32))
        assert np.array_equal(t.get_accumulators(), np.zeros_like(theta))
        # with accumulators loaded by an ordinary step (the weights put back): the weights stay, the accumulators decay by rho
        t.step(ordinary, 0.0, 0, 1, beta, 1e-3, rho, 1e-7, 0)
        loaded = t.get_accumulators()
        assert np.count_nonzero(loaded) >= loaded.size / 2 and not np.array_equal(t.get_weights(), theta)
        t.set_weights(theta)
        t.step(certain, 0.0, 0, 2, beta, 1e-3, rho, 1e-7, 0)
        assert np.array_equal(t.get_weights().view(np.uint32), theta.view(np.uint32))
        decayed = (np.float64(np.float32(rho)) * loaded.astype(np.float64)).astype(np.float32)   # train_rmsprop with g = 0
        assert np.array_equal(t.get_accumulators().view(np.uint32), decayed.view(np.uint32))
    finally:
        t.close()


def test_forward_only_paths_agree_in_saturation(stock_weights):
    batch = saturated_batch(stock_weights, SAT_N, ALL_BUT_EDGE)
    weights, x, y = batch['weights'], batch['x'], saturated_targets('random', SAT_N)
    single, group = _lib.HipTrainer(weights, 29, 13), _lib.HipTrainer([weights], 29, 13)
    try:
        loss, _, probs = single.loss_grad(x, y, loss_bias=0.7)
        check_probabilities_in_bands(probs, batch['p'], batch['bands'])
        group.set_data(x[::-1], y[::-1])
        rows = np.arange(SAT_N - 1, -1, -1, dtype=np.int32)
        results = {'evaluate': single.evaluate(x, y, loss_bias=0.7)}
        for name, (l, a, p) in (('evaluate_models', group.evaluate_models(x, y, loss_bias=0.7)),
                                ('evaluate_indices', group.evaluate_indices(rows, loss_bias=0.7))):
            assert l.shape == a.shape == (1,) and p.shape == (1, SAT_N)
            results[name] = (float(l[0]), float(a[0]), p[0])
    finally:
        single.close()
        group.close()
    want_acc = float(np.float32(np.mean(np.rint(probs) == y)))                   # (acc_out is a float32)
    for name, (l, a, p) in results.items():
        print('%s: loss %.7g against %.7g, accuracy %.6g' % (name, l, loss, a))
        assert np.array_equal(p.view(np.uint32), probs.view(np.uint32)), name
        assert rel_err(l, loss) <= SAT_LOSS_REL_TOL, name
        assert a == want_acc, name


def test_saturated_head_beside_other_networks(stock_weights):
    """test_train_models.test_alone_equals_together on a batch whose tiles mix zero-gradient and ordinary samples"""
    batch = saturated_batch(stock_weights, SAT_N, ALL_BUT_EDGE)
    x, y = batch['x'], saturated_targets('random', SAT_N)
    tiles = batch['bands'].reshape(-1, 16)
    assert sum(('one' in tile) and ('mid' in tile) for tile in tiles) >= len(tiles) / 2
    models = [synth.make_weights(13, (8,), seed=3), batch['weights']]
    hp = dict(dropout_rate=(0.2, 0.0), seed=(7, 8), loss_bias=(0.3, 0.7), lr=(1e-3, 1e-3))
    idx = np.arange(SAT_N, dtype=np.int32)
    alone = []
    for m, w in enumerate(models):
        t = _lib.HipTrainer(w, 29, 13)
        t.set_data(x, y)
        loss = t.step(idx, hp['dropout_rate'][m], hp['seed'][m], 4, hp['loss_bias'][m], hp['lr'][m], 0.9, 1e-7, 0)
        alone.append((np.float32(loss), t.get_weights(), t.get_accumulators()))
        t.close()
    g = _lib.HipTrainer(models, 29, 13)
    g.set_data(x, y)
    losses = g.step_models(idx, step=4, rho=0.9, eps=1e-7, **hp)
    theta, accum = g.split(g.get_weights()), g.split(g.get_accumulators())
    g.close()
    for m, (loss, w, a) in enumerate(alone):
        assert np.isfinite(loss) and np.all(np.isfinite(w)) and a.any()
        assert np.float32(losses[m]).view(np.uint32) == loss.view(np.uint32), m
        assert np.array_equal(theta[m].view(np.uint32), w.view(np.uint32)), m
        assert np.array_equal(accum[m].view(np.uint32), a.view(np.uint32)), m


def saturated_floors(stock_weights):
    """CPU only: the float32 floors the SAT_* bounds are 20x of, over the cases of test_gradients_saturated_head, with
    torch float32 in the kernel's place (its probabilities enter head32 as the kernel's do).  Not a test:
    ``PYTHONPATH=. python tests/test_train.py`` prints them."""
    import torch
    floors = {}
    for targets, loss_bias, rate in SAT_CASES:
        batch = saturated_batch(stock_weights, SAT_N, ALL_BUT_EDGE, rate)
        weights, x, masks, y = batch['weights'], batch['x'], batch['masks'], saturated_targets(targets, SAT_N)
        p32 = ref.forward_numpy(weights, x, masks, dtype=torch.float32)['p'].astype(np.float32)
        low = (batch['bands'] == 'neg') | (batch['bands'] == 'neg_sat')
        prob = float((np.abs(p32.astype(np.float64) - batch['p']) / batch['p'])[low].max())
        ds = ref.head32(p32, y, loss_bias, SAT_N)[0]
        g64, g32 = ref.grads_from_ds(weights, x, masks, ds), ref.grads_from_ds(weights, x, masks, ds, dtype=torch.float32)
        grad = max(float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in ref.NAMES if g64[k].any()) if ds.any() else 0.0
        tp, ty, eps, b = torch.tensor(p32), torch.tensor(y), torch.tensor(np.float32(ref.EPS)), torch.tensor(np.float32(loss_bias))
        loss32 = b * (-(1 - ty) * torch.log((1 - tp) + eps)).mean() + (1 - b) * (-ty * torch.log(tp + eps)).mean()
        loss = rel_err(float(loss32), ref.head32_loss(p32, y, loss_bias))
        print('%-6s bias %g rate %g: probabilities (neg, neg_sat) %.3g, gradients %.3g, loss %.3g' %
              (targets, loss_bias, rate, prob, grad, loss))
        key = 'masks' if rate > 0 else 'plain'
        floors[key] = [max(u, v) for u, v in zip(floors.get(key, (0.0, 0.0, 0.0)), (prob, grad, loss))]
    return floors


def test_unsupported_shapes_are_refused_by_name():
    for weights, T, F, field in ((synth.make_weights(13, (20, 20)), 29, 13, 'n_layers'),
                                 (synth.make_weights(13, (33,)), 29, 13, 'units'),
                                 (synth.make_weights(13, (20,)), 65, 13, 'n_features')):
        with pytest.raises(NotImplementedError, match=field):
            _lib.HipTrainer(weights, T, F)


def ptr(a):
    return None if a is None else a.ctypes.data


def test_argument_errors_leave_the_outputs_untouched(stock_weights):
    lib = _lib.load()
    t = _lib.HipTrainer(stock_weights, 29, 13)
    x = candidates('n01', 4)
    y = np.array([0, 1, 0, 1], dtype=np.float32)
    bad_y = np.array([0, 1, 1.5, 1], dtype=np.float32)
    nan_y = np.array([0, np.nan, 1, 1], dtype=np.float32)
    sentinel = np.float32(-77.0)
    loss, acc = np.full(1, sentinel), np.full(1, sentinel)
    grads = np.full(t.n_params, sentinel)
    probs = np.full(4, sentinel)
    theta = t.get_weights()

    def loss_grad(x_, y_, n, loss_, grads_):
        return lib.pe_trainer_loss_grad(t._h, ptr(x_), ptr(y_), n, None, 0.7, ptr(loss_), ptr(grads_), ptr(probs))

    def evaluate(x_, y_, n):
        return lib.pe_trainer_evaluate(t._h, ptr(x_), ptr(y_), n, 0.7, ptr(loss), ptr(acc), ptr(probs))

    def step(idx_, n, rate, loss_=loss):
        return lib.pe_trainer_step(t._h, ptr(idx_), n, rate, 1, 0, 0.7, 1e-3, 0.9, 1e-7, 0, ptr(loss_))

    idx = np.array([0, 1, 2, 3], dtype=np.int32)
    calls = [loss_grad(None, y, 4, loss, grads), loss_grad(x, None, 4, loss, grads), loss_grad(x, y, 4, None, grads),
             loss_grad(x, y, 4, loss, None), loss_grad(x, y, 0, loss, grads), loss_grad(x, y, -3, loss, grads),
             loss_grad(x, bad_y, 4, loss, grads), loss_grad(x, nan_y, 4, loss, grads),
             evaluate(None, y, 4), evaluate(x, None, 4), evaluate(x, y, 0), evaluate(x, bad_y, 4),
             lib.pe_trainer_set_data(t._h, ptr(x), ptr(bad_y), 4), lib.pe_trainer_set_data(t._h, ptr(x), ptr(y), 0),
             lib.pe_trainer_set_data(t._h, None, ptr(y), 4), lib.pe_trainer_apply(t._h, None, 1e-3, 0.9, 1e-7, 0),
             step(idx, 4, 0.2)]                                           # (no dataset yet)
    t.set_data(x, y)
    calls += [step(np.array([0, 1, 4, 3], dtype=np.int32), 4, 0.2), step(np.array([0, -1, 2, 3], dtype=np.int32), 4, 0.2),
              step(idx, 4, 1.0), step(idx, 4, -0.5), step(idx, 4, float('nan')), step(idx, 0, 0.2), step(None, 4, 0.2),
              step(idx, 4, 0.2, None)]
    assert calls == [_lib.PE_ERR_INVALID] * len(calls)
    assert lib.pe_trainer_last_error(t._h)
    for out in (loss, acc, grads, probs):
        assert np.all(out == sentinel)
    assert np.array_equal(t.get_weights(), theta) and not t.get_accumulators().any()
    with pytest.raises(ValueError, match='outside'):
        t.loss_grad(x, bad_y)
    t.close()


def ulps(got, want64):
    want32 = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want32)).astype(np.float64)


def test_rmsprop_apply_matches_the_formula(stock_weights):
    t = _lib.HipTrainer(stock_weights, 29, 13)
    n, n_gru = t.n_params, (13 + 20 + 1) * 60
    rng = np.random.default_rng(2)
    lr, rho, eps = np.float32(1e-3), np.float32(0.9), np.float32(1e-7)
    theta = t.get_weights().astype(np.float64)
    accum = np.zeros(n)
    for call in range(3):
        g = rng.normal(0.0, 0.05, n).astype(np.float32)
        g[rng.random(n) < 0.1] = 0.0
        tiny = rng.random(n) < 0.1
        g[tiny] = (rng.normal(0.0, 1e-8, n).astype(np.float32))[tiny]
        t.apply(g, lr, rho, eps)
        theta, accum = ref.rmsprop(theta, accum, g.astype(np.float64), float(lr), float(rho), float(eps))
        got_theta, got_accum = t.get_weights(), t.get_accumulators()
        u_t, u_a = float(ulps(got_theta, theta).max()), float(ulps(got_accum, accum).max())
        print('call %d: parameters %.2f ulp, accumulators %.2f ulp' % (call, u_t, u_a))
        assert u_t <= 4 and u_a <= 4
        theta, accum = got_theta.astype(np.float64), got_accum.astype(np.float64)     # the state is float32 between calls
    # frozen layers keep parameters and accumulators bit for bit
    g = rng.normal(0.0, 0.05, n).astype(np.float32)
    for mask, frozen in ((1, slice(0, n_gru)), (2, slice(n_gru, n)), (3, slice(0, n))):
        before_t, before_a = t.get_weights(), t.get_accumulators()
        t.apply(g, lr, rho, eps, frozen_mask=mask)
        after_t, after_a = t.get_weights(), t.get_accumulators()
        assert np.array_equal(before_t[frozen].view(np.uint32), after_t[frozen].view(np.uint32))
        assert np.array_equal(before_a[frozen].view(np.uint32), after_a[frozen].view(np.uint32))
        moved = np.ones(n, dtype=bool)
        moved[frozen] = False
        assert np.all(before_a[moved] != after_a[moved])
    t.reset_optimizer()
    assert not t.get_accumulators().any()
    t.close()


@pytest.mark.parametrize('n', [33, 240])
def test_fused_step_is_gradient_then_apply(stock_weights, n):
    rng = np.random.default_rng(n)
    data = candidates('n03', 300, seed=21)
    labels = targets_for(300, 21)
    idx = rng.permutation(300)[:n].astype(np.int32)
    seed, step, rate = 99, 5, 0.2
    fused = _lib.HipTrainer(stock_weights, 29, 13)
    fused.set_data(data, labels)
    manual = _lib.HipTrainer(stock_weights, 29, 13)
    for k in range(2):                      # two steps: the second starts from non-zero accumulators
        loss_f = fused.step(idx, rate, seed, step + k, 0.7, 1e-3, 0.9, 1e-7, 0)
        masks = _lib.dropout_masks(seed, step + k, n, 13, rate)
        loss_m, grads, _ = manual.loss_grad(data[idx], labels[idx], masks=masks, loss_bias=0.7)
        manual.apply(grads, 1e-3, 0.9, 1e-7, 0)
        assert np.float32(loss_f).view(np.uint32) == np.float32(loss_m).view(np.uint32)
        assert np.array_equal(fused.get_weights().view(np.uint32), manual.get_weights().view(np.uint32))
        assert np.array_equal(fused.get_accumulators().view(np.uint32), manual.get_accumulators().view(np.uint32))
    assert fused.get_accumulators().any()
    fused.close()
    manual.close()


def test_predict_and_evaluate_match_the_inference_engine(stock_weights):
    from mycroft_precise_amd.train import Trainer
    x = candidates('mfcc', 100)
    y = targets_for(100)
    eng = _lib.HipEngine(pr, stock_weights, n_streams=1)
    want = eng.predict(x)
    eng.close()
    tr = Trainer(weights=stock_weights)
    got = tr.predict(x)
    loss, acc = tr.evaluate(x, y.reshape(-1, 1))
    tr.close()
    assert got.shape == want.shape == (100, 1)
    err = float(np.abs(got - want).max())
    print('trainer predict vs engine predict: %.3g' % err)
    assert err <= 1e-5
    res = ref.loss_and_grads(stock_weights, x, y)
    assert abs(loss - res['loss']) <= 1e-5
    assert acc == float(np.float32(np.mean(np.rint(got.reshape(-1)) == y)))        # (acc_out is a float32)


def learning_task(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (n, 29, 13)).astype(np.float32)
    y = (rng.random(n) < 0.5).astype(np.float32)
    x[y > 0, 12:20, 2:5] += np.float32(1.5)
    return x, y


def reference_training(weights, x, y, xv, yv, batch, epochs, rate, loss_bias, seed):
    """the same loop in float64 on the CPU: the same masks, torch autograd, the RMSprop formula"""
    import torch
    params = ref.tensors(weights)
    accum = [np.zeros(tuple(p.shape)) for p in params]
    step = 0
    for _ in range(epochs):
        for a in range(0, len(x), batch):
            xb, yb = x[a:a + batch], y[a:a + batch]
            masks = _lib.dropout_masks(seed, step, len(xb), x.shape[2], rate)
            loss, _ = ref.loss_fn(params, xb, yb, masks, loss_bias)
            grads = torch.autograd.grad(loss, params)
            with torch.no_grad():
                for i, (p, g) in enumerate(zip(params, grads)):
                    new, accum[i] = ref.rmsprop(p.numpy(), accum[i], g.numpy())
                    p.copy_(torch.from_numpy(new))
            step += 1
    with torch.no_grad():
        loss, out = ref.loss_fn(params, xv, yv, None, loss_bias)
    return float(loss), float(np.mean(np.rint(out['p'].numpy()) == yv))


def test_training_learns_like_the_reference_trainer():
    from mycroft_precise_amd.train import Trainer
    x, y = learning_task(512, 1)
    xv, yv = learning_task(256, 2)
    weights = synth.make_weights(13, (20,), seed=5)
    tr = Trainer(weights=weights, params=ModelParams(dropout=0.2, loss_bias=0.7), seed=17)
    start = tr.evaluate(xv, yv)[0]
    hist = tr.fit(x, y, batch_size=128, epochs=30, validation_data=(xv, yv), shuffle=False)
    tr.close()
    want_loss, want_acc = reference_training(weights, x, y, xv, yv, 128, 30, 0.2, 0.7, 17)
    got_loss, got_acc = hist['val_loss'][-1], hist['val_acc'][-1]
    print('validation loss %.4f -> %.5f (reference trainer %.5f, difference %.2f %%), accuracy %.4f (reference %.4f)' %
          (start, got_loss, want_loss, 100 * abs(got_loss - want_loss) / want_loss, got_acc, want_acc))
    assert len(hist['loss']) == 30 and hist['loss'][-1] < hist['loss'][0]
    assert got_loss <= 0.05
    assert got_acc >= 0.97
    assert abs(got_loss - want_loss) <= 0.05 * want_loss


def test_trained_model_round_trip(tmp_path, stock_weights):
    from mycroft_precise_amd.network_runner import HipRunner
    from mycroft_precise_amd.train import Trainer
    x, y = learning_task(64, 3)
    tr = Trainer(weights=stock_weights, seed=1)
    tr.fit(x, y, batch_size=32, epochs=2)
    path = str(tmp_path / 'trained.npz')
    tr.save(path)
    want = tr.predict(x)
    weights = tr.weights
    tr.close()
    loaded = load_weights(path)
    for a, b in zip(loaded['gru'][0] + (loaded['dense_kernel'], loaded['dense_bias']),
                    weights['gru'][0] + (weights['dense_kernel'], weights['dense_bias'])):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert any(not np.array_equal(a, b) for a, b in zip(loaded['gru'][0], stock_weights['gru'][0]))
    got = HipRunner(path).predict(x)
    assert float(np.abs(got - want).max()) <= 1e-5


if __name__ == '__main__':
    from conftest import golden
    stock = golden('weights_stock_seed42.npz')
    for name, (prob, grad, loss) in saturated_floors({'gru': [(stock['kernel'], stock['recurrent_kernel'], stock['bias'])],
                                                      'dense_kernel': stock['dense_kernel'],
                                                      'dense_bias': stock['dense_bias']}).items():
        print('%s: float32 floors: probabilities %.3g, gradients %.3g, loss %.3g; 20x: %.3g, %.3g, %.3g' %
              (name, prob, grad, loss, 20 * prob, 20 * grad, 20 * loss))
