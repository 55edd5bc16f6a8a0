"""GPU: training of stacked two-layer networks (pe_trainer_create_stacked, csrc/gru_train_stacked_device.h)
against the float64 autograd reference of train_stacked_reference.py, and the bit-level properties of the stacked path.

Bounds: GRAD_TOL = 1e-5 (per tensor max|d| / max|reference tensor|), LOSS_TOL = 1e-6, PROB_TOL = 1e-5: 20x the float32 floor,
which is torch float32 autograd against the same float64 reference (train_stacked_reference.loss_and_grads(dtype=float32))
measured on the CPU over every case of CASES below, with the project's mask function for both layers
(the comment above GRAD_TOL_OF holds the figures).  The three bounds carry over wherever the floor of a case stays <= 5.4e-7 for the
gradients (the top of the band they were derived from); a case above that is named in GRAD_TOL_OF with 20x its
own measured floor.  No bound comes from the kernel's output.

Every batch is built from kink-safe candidates (both layers' gate pre-activations at least 1e-3 from +-2.5 and |logit| <= 8
in float64) and every pool asserts that at least half of its candidates pass.  The 'n03', T = 3 pools assert saturated and
unsaturated gates in layer 0; (20, 20), (33, 33) and the pool with layer 1's kernel scaled assert the same in layer 1.
"""
import functools

import numpy as np
import pytest

import test_train as tt
import train_stacked_reference as ref
from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.model import ModelParams, load_weights
from mycroft_precise_amd.train import flatten_weights

pytestmark = pytest.mark.gpu

GRAD_TOL, LOSS_TOL, PROB_TOL = tt.GRAD_TOL, tt.LOSS_TOL, tt.PROB_TOL
TILE = 16
WIDTHS = ((1, 1), (20, 20), (33, 33), (16, 48), (64, 64), (40, 200), (200, 40), (256, 256))

# The measured float32 floor, per family of CASES (gradients: worst tensor; loss; probabilities):
#   edge-*      (T = 3, 'n03', rate 0.2, n in 1, 15, 16, 17, 33)   gradients 2.4e-7 .. 5.2e-7 but for the cases listed below,
#               loss <= 1.2e-7 (n = 1: one sample's float32 log), probabilities <= 1.6e-7
#   chain-*     2.3e-7 .. 4.9e-7, loss <= 4.9e-8, probabilities <= 5.5e-8
#   shape-*     4.0e-7, 4.6e-7 and 5.8e-7 at T = 64, F = 32, (256, 256); loss <= 2.4e-8, probabilities <= 6.4e-8
#   bias-*, targets-*, no-masks   2.2e-7 .. 4.2e-7, loss <= 3.7e-8, probabilities <= 1.1e-7
#   scaled-layer1-64x64           3.8e-7, loss 1.6e-7, probabilities 3.2e-7
#   258-tiles-64x33               3.2e-7, loss 1.1e-8, probabilities 1.2e-7
# PROB_TOL = 1e-5 is above 20x every probability floor.  LOSS_TOL = 1e-6 is BELOW 20x the loss floor of the n = 1 cases
# (1.2e-7) and of the scaled case (1.6e-7); the tighter 1e-6 is kept for every case.
# Cases whose gradient floor exceeds 5.4e-7 -> 20 x their own floor.  (1, 1): one unit per layer, every tensor a handful of
# numbers whose largest entry is itself a cancelling sum; (16, 48) from n = 16, (256, 256) at n = 15..17: the worst tensor is dense_bias or
# bias_1, ONE sum of ds over the batch that nearly cancels, so its float32 error is large against its own size.
GRAD_TOL_OF = {
    'edge-1x1-n15': 20 * 1.73e-6, 'edge-1x1-n16': 20 * 1.40e-6, 'edge-1x1-n17': 20 * 1.33e-6, 'edge-1x1-n33': 20 * 1.26e-6,
    'edge-16x48-n16': 20 * 1.08e-6, 'edge-16x48-n17': 20 * 1.22e-6, 'edge-16x48-n33': 20 * 1.29e-6,
    'edge-40x200-n16': 20 * 5.61e-7,
    'edge-256x256-n15': 20 * 8.01e-6, 'edge-256x256-n16': 20 * 1.97e-6, 'edge-256x256-n17': 20 * 1.09e-6,
    'shape-T64-F32-256x256': 20 * 5.78e-7,
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def stacked_weights(F, units, seed=0, scale1=1.0):
    w = synth.make_weights(F, units) if seed == 0 else synth.make_weights(F, units, seed=seed)
    if scale1 != 1.0 and len(units) == 2:
        k1, rk1, b1 = w['gru'][1]
        w = dict(w, gru=[w['gru'][0], ((k1 * np.float32(scale1)).astype(np.float32), rk1, b1)])
    return w


def masks_for(seed, step, n, F, H1, rate):
    return (_lib.dropout_masks(seed, step, n, F, rate), _lib.dropout_masks(seed, step, n, H1, rate, layer=1))


@functools.lru_cache(maxsize=None)
def pool(units, family, T=3, F=13, rate=0.2, seed=None, n=33, n_candidates=256, scale1=1.0, saturated=(0,)):
    """-> (weights, x [n, T, F], masks (m0, m1) or None): the first n kink-safe candidates; ``saturated``: the layers whose
    kept samples must hold gate values on both sides of the hard sigmoid's kinks"""
    seed = sum(units) + T if seed is None else seed
    w = stacked_weights(F, units, 0, scale1)
    x = tt.candidates(family, n_candidates, T, F, seed)
    masks = masks_for(seed, 1, n_candidates, F, units[0], rate) if rate > 0 else None
    out = ref.forward_numpy(w, x, masks)
    keep = np.flatnonzero(ref.kink_safe(out))
    print('%s %s T=%d F=%d: %d of %d candidates kink-safe' % (family, units, T, F, keep.size, n_candidates))
    assert keep.size >= n_candidates / 2 and keep.size >= n
    keep = keep[:n]
    for layer in saturated:
        a = np.abs(np.concatenate([out['a_z'][layer][:, keep], out['a_r'][layer][:, keep]], axis=2))
        assert (a > 2.5).any() and (a < 2.5).any(), (units, layer)
    return w, x[keep], (tuple(m[:, keep] for m in masks) if masks is not None else None)


def n03_pool(units):
    return pool(units, 'n03', saturated=(0, 1) if units in ((20, 20), (33, 33)) else (0,))


def scaled_pool():
    """(64, 64) with layer 1's input kernel four times as large: layer 1 saturates too"""
    return pool((64, 64), 'n03', seed=77, scale1=4.0, saturated=(0, 1))


def case(builder, n=None, targets=None, loss_bias=0.7, seed=0):
    def make():
        w, x, masks = builder()
        k = len(x) if n is None else n
        y = tt.targets_for(k, seed) if targets is None else np.full(k, targets, dtype=np.float32)
        return dict(weights=w, x=x[:k], y=y, masks=None if masks is None else tuple(m[:, :k] for m in masks), loss_bias=loss_bias)
    return make


CASES = {}
for _u in WIDTHS:
    for _n in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        CASES['edge-%dx%d-n%d' % (_u + (_n,))] = case(functools.partial(n03_pool, _u), n=_n, seed=sum(_u))
for _u in ((33, 33), (128, 128)):
    for _T in (1, 2, 29):
        CASES['chain-%dx%d-T%d' % (_u + (_T,))] = case(functools.partial(pool, _u, 'n01', T=_T, saturated=()), seed=_T)
for _T, _F, _u, _s in ((64, 32, (256, 256), 5), (29, 26, (128, 64), 7), (29, 1, (33, 40), 9)):
    CASES['shape-T%d-F%d-%dx%d' % ((_T, _F) + _u)] = case(functools.partial(pool, _u, 'n01', T=_T, F=_F, seed=_s, saturated=()), seed=_T)
for _b in (0.0, 0.7, 1.0):
    CASES['bias-%g' % _b] = case(functools.partial(n03_pool, (33, 33)), loss_bias=_b, seed=5)
for _y in (0.0, 1.0):
    CASES['targets-%g' % _y] = case(functools.partial(n03_pool, (33, 33)), targets=_y)
CASES['no-masks-20x20'] = case(functools.partial(pool, (20, 20), 'n03', rate=0.0, seed=12, saturated=(0, 1)), seed=12)
CASES['scaled-layer1-64x64'] = case(scaled_pool, seed=77)
# 258 tiles for 256 compute units, the last tile one sample; 64 gradient chunks of 116 or 117 records
CASES['258-tiles-64x33'] = case(functools.partial(pool, (64, 33), 'n01', T=29, rate=0.2, seed=11, n=257 * TILE + 1, n_candidates=4400,
                                                  saturated=()), seed=11)


def errors(got, want):
    """(loss, flat gradients, probabilities) against a reference result -> ({tensor: relative error}, d_loss, d_prob)"""
    loss, grads, probs = got
    sizes = np.cumsum([g.size for g in want['grads'].values()])[:-1]
    worst = {}
    for (name, wg), g in zip(want['grads'].items(), np.split(np.asarray(grads, dtype=np.float64), sizes)):
        wg = wg.reshape(-1)
        scale = float(np.abs(wg).max())
        worst[name] = float(np.abs(g - wg).max()) / scale if scale > 0 else float(np.abs(g).max())
    return worst, abs(loss - want['loss']), float(np.abs(probs - want['p']).max())


def check_against_reference(label, c, grad_tol=GRAD_TOL):
    w, x, y, masks, loss_bias = c['weights'], c['x'], c['y'], c['masks'], c['loss_bias']
    T, F = x.shape[1], x.shape[2]
    want = ref.loss_and_grads(w, x, y, masks, loss_bias)
    t = _lib.HipTrainer(w, T, F, stacked=True)
    try:
        got = t.loss_grad(x, y, masks=masks, loss_bias=loss_bias)
        again = t.loss_grad(x, y, masks=masks, loss_bias=loss_bias)
    finally:
        t.close()
    assert got[0] == again[0] and np.array_equal(bits(got[1]), bits(again[1])) and np.array_equal(bits(got[2]), bits(again[2]))
    worst, d_loss, d_prob = errors(got, want)
    print('%s N=%d T=%d F=%d bias=%g: grads %s loss %.3g probs %.3g' %
          (label, len(x), T, F, loss_bias, ' '.join('%s %.3g' % kv for kv in worst.items()), d_loss, d_prob))
    assert max(worst.values()) <= grad_tol, worst
    assert d_loss <= LOSS_TOL
    assert d_prob <= PROB_TOL


# ---- 1. gradients, loss and probabilities against float64 ----------------------------------------------------------------
@pytest.mark.parametrize('label', list(CASES))
def test_gradients_against_float64(label):
    check_against_reference(label, CASES[label](), GRAD_TOL_OF.get(label, GRAD_TOL))


# ---- 2. bit-level properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('units,n', [((40, 33), 33), ((40, 33), 240), ((128, 128), 33), ((20, 200), 49)])
def test_step_is_gradient_then_apply_and_repeats(units, n):
    """generated masks: pe_trainer_step against pe_trainer_loss_grad with the host's masks of both layers, then pe_trainer_apply;
    the first step's loss also against the float64 reference under the restated mask function"""
    w = stacked_weights(13, units)
    data, labels = tt.candidates('n03', 300, seed=21), tt.targets_for(300, 21)
    idx = np.random.default_rng(n + sum(units)).permutation(300)[:n].astype(np.int32)
    seed, step, rate = 99, 5, 0.2
    fused, again, manual = (_lib.HipTrainer(w, 29, 13, stacked=True) for _ in range(3))
    try:
        fused.set_data(data, labels)
        again.set_data(data, labels)
        for k in range(2):                      # two steps: the second starts from non-zero accumulators
            loss_f = fused.step(idx, rate, seed, step + k, 0.7, 1e-3, 0.9, 1e-7, 0)
            loss_a = again.step(idx, rate, seed, step + k, 0.7, 1e-3, 0.9, 1e-7, 0)
            masks = masks_for(seed, step + k, n, 13, units[0], rate)
            loss_m, grads, probs = manual.loss_grad(data[idx], labels[idx], masks=masks, loss_bias=0.7)
            if k == 0:
                restated = (ref.mask_function(seed, step, n, 13, rate, 0), ref.mask_function(seed, step, n, units[0], rate, 1))
                out = ref.forward_numpy(w, data[idx], restated)
                mid = np.abs(out['logit']) <= 8.0
                assert mid.sum() >= n / 2
                assert float(np.abs(probs - out['p'])[mid].max()) <= 1e-3         # (kinks may flip: the masks are what is checked)
            manual.apply(grads, 1e-3, 0.9, 1e-7, 0)
            for other, loss_o in ((again, loss_a), (manual, loss_m)):
                assert np.float32(loss_f).view(np.uint32) == np.float32(loss_o).view(np.uint32)
                assert np.array_equal(bits(fused.get_weights()), bits(other.get_weights()))
                assert np.array_equal(bits(fused.get_accumulators()), bits(other.get_accumulators()))
        assert fused.get_accumulators().all() and not np.array_equal(fused.get_weights(), flatten_weights(w))
    finally:
        for t in (fused, again, manual):
            t.close()


GROUP_UNITS = ((20,), (40, 33), (128,), (64, 64), (40, 33))


@pytest.mark.parametrize('n', [33, 240])
def test_alone_equals_together_in_a_mixed_group(n):
    """each network of a (one-layer, stacked, wide, stacked, stacked) trainer against a trainer of its own, in two orders; the
    one-layer members also against a pe_trainer_create_wide trainer"""
    models = [stacked_weights(13, u, seed=10 + i) for i, u in enumerate(GROUP_UNITS)]
    data, labels = tt.candidates('n03', 300, seed=22), tt.targets_for(300, 22)
    idx = np.random.default_rng(n).permutation(300)[:n].astype(np.int32)
    hp = dict(dropout_rate=(0.2, 0.0, 0.2, 0.2, 0.3), seed=(7, 8, 9, 10, 11), loss_bias=(0.3, 0.7, 0.7, 0.5, 0.9),
              lr=(1e-3, 2e-3, 1e-3, 5e-4, 1e-3), frozen_mask=(0, 2, 0, 4, 0))

    def alone(m, **kind):
        t = _lib.HipTrainer(models[m], 29, 13, **kind)
        t.set_data(data, labels)
        losses = [np.float32(t.step(idx, hp['dropout_rate'][m], hp['seed'][m], 4 + k, hp['loss_bias'][m], hp['lr'][m], 0.9, 1e-7,
                                    hp['frozen_mask'][m])) for k in range(2)]
        out = (losses, t.get_weights(), t.get_accumulators(), t.evaluate(data[:n])[2])
        t.close()
        return out

    def together(order):
        g = _lib.HipTrainer([models[m] for m in order], 29, 13, stacked=True)
        g.set_data(data, labels)
        sub = {k: tuple(v[m] for m in order) for k, v in hp.items()}
        losses = [g.step_models(idx, step=4 + k, rho=0.9, eps=1e-7, **sub) for k in range(2)]
        out = (losses, g.split(g.get_weights()), g.split(g.get_accumulators()), g.evaluate_models(data[:n])[2])
        g.close()
        return out

    singles = [alone(m, stacked=True) for m in range(len(models))]
    for order in ((0, 1, 2, 3, 4), (3, 4, 0, 2, 1)):
        losses, theta, accum, probs = together(order)
        for pos, m in enumerate(order):
            want = singles[m]
            for k in range(2):
                assert np.float32(losses[k][pos]).view(np.uint32) == want[0][k].view(np.uint32), (order, m, k)
            assert np.array_equal(bits(theta[pos]), bits(want[1])), (order, m)
            assert np.array_equal(bits(accum[pos]), bits(want[2])), (order, m)
            assert np.array_equal(bits(probs[pos]), bits(want[3])), (order, m)
    assert not np.array_equal(bits(singles[1][1]), bits(singles[4][1]))           # the two (40, 33) differ by seed and rate
    for m, u in enumerate(GROUP_UNITS):
        if len(u) == 1:
            wide = alone(m, wide=True)
            assert [v.view(np.uint32) for v in wide[0]] == [v.view(np.uint32) for v in singles[m][0]]
            for a, b in zip(wide[1:], singles[m][1:]):
                assert np.array_equal(bits(a), bits(b)), m


@pytest.mark.parametrize('units', [(40, 33), (128, 72)])
def test_one_forward(units):
    """every forward-only path, and loss_grad's probabilities without masks, give the same bits"""
    n = 240
    w = stacked_weights(13, units)
    x, y = tt.candidates('n03', n, seed=23), tt.targets_for(n, 23)
    rows = np.random.default_rng(sum(units)).permutation(n).astype(np.int32)
    t = _lib.HipTrainer([w], 29, 13, stacked=True)
    one = _lib.HipTrainer(w, 29, 13, stacked=True)
    try:
        t.set_data(x, y)
        t.set_validation(x[::-1], y[::-1])
        want = t.evaluate_models(x, y)[2][0]
        assert np.array_equal(bits(one.loss_grad(x, y)[2]), bits(want))
        assert np.array_equal(bits(one.evaluate(x, y)[2]), bits(want))
        assert np.array_equal(bits(t.evaluate_models(source='data')[2][0]), bits(want))
        assert np.array_equal(bits(t.evaluate_models(source='validation')[2][0]), bits(want[::-1]))
        assert np.array_equal(bits(t.evaluate_indices(rows)[2][0]), bits(want[rows]))
        assert np.array_equal(bits(t.stats_models(thresholds=(0.5,), source='data', want_probs=True)[2][0]), bits(want))
        assert np.array_equal(bits(t.stats_models(x, y, thresholds=(0.5,), source='host', want_probs=True)[2][0]), bits(want))
        assert np.array_equal(bits(t.sample_choose(5, 'error', want_probs=True)[2]), bits(want))
        assert np.array_equal(bits(t.evaluate_models(x, y)[2][0]), bits(want))
    finally:
        t.close()
        one.close()
    out = ref.forward_numpy(w, x)
    mid = np.abs(out['logit']) <= 8.0
    assert mid.sum() >= n / 2 and float(np.median(np.abs(want - out['p'])[mid])) <= PROB_TOL


# ---- 3. padding and stale scratch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('units', [(33, 100), (100, 33)])
def test_stale_scratch_is_never_read(units):
    """A short call after a larger call with larger values on the same trainer: records, dx, masks, D, partials and chunk
    partials then hold what the larger call left; the result is the fresh trainer's in bits."""
    w = stacked_weights(13, units)
    big = tt.candidates('n03', 80, seed=sum(units)) * np.float32(10.0)
    small = tt.candidates('n01', TILE + 1, seed=sum(units) + 1)
    y_big, y_small = tt.targets_for(80, 1), tt.targets_for(TILE + 1, 2)
    masks = masks_for(3, 0, TILE + 1, 13, units[0], 0.2)
    idx_big, idx_small = np.arange(80, dtype=np.int32), np.arange(80, 80 + TILE + 1, dtype=np.int32)
    used, fresh = _lib.HipTrainer(w, 29, 13, stacked=True), _lib.HipTrainer(w, 29, 13, stacked=True)
    try:
        theta = used.get_weights()
        for t in (used, fresh):
            t.set_data(np.concatenate([big, small]), np.concatenate([y_big, y_small]))
        used.loss_grad(big, y_big)
        used.step(idx_big, 0.2, 1, 0, 0.7, 1e-3, 0.9, 1e-7, 0)
        used.evaluate(big, y_big)
        used.set_weights(theta)
        used.reset_optimizer()
        got, want = used.loss_grad(small, y_small, masks=masks), fresh.loss_grad(small, y_small, masks=masks)
        assert np.float32(got[0]).view(np.uint32) == np.float32(want[0]).view(np.uint32)
        assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(bits(got[2]), bits(want[2]))
        assert np.all(np.isfinite(got[1])) and got[1].any()
        losses = [t.step(idx_small, 0.2, 1, 1, 0.7, 1e-3, 0.9, 1e-7, 0) for t in (used, fresh)]
        assert np.float32(losses[0]).view(np.uint32) == np.float32(losses[1]).view(np.uint32)
        assert np.array_equal(bits(used.get_weights()), bits(fresh.get_weights()))
        assert np.array_equal(bits(used.get_accumulators()), bits(fresh.get_accumulators()))
        assert np.array_equal(bits(used.evaluate(small)[2]), bits(fresh.evaluate(small)[2]))
    finally:
        used.close()
        fresh.close()


# ---- 4. frozen layers ------------------------------------------------------------------------------------------------------
def blocks(F, units):
    """the three slices of the flat vector: GRU 0, GRU 1, Dense"""
    n0, n1 = (F + units[0] + 1) * 3 * units[0], (units[0] + units[1] + 1) * 3 * units[1]
    return slice(0, n0), slice(n0, n0 + n1), slice(n0 + n1, n0 + n1 + units[1] + 1)


@pytest.mark.parametrize('frozen_mask', [1, 2, 4, 7, 0])
def test_frozen_bits_keep_parameters_and_accumulators(frozen_mask):
    units = (40, 24)
    w = stacked_weights(13, units)
    x, y = tt.learning_task(40, 4)
    t = _lib.HipTrainer(w, 29, 13, stacked=True)
    try:
        t.set_data(x, y)
        t.step(np.arange(40, dtype=np.int32), 0.2, 1, 0, 0.7, 1e-3, 0.9, 1e-7, 0)      # accumulators away from zero
        before_t, before_a = t.get_weights(), t.get_accumulators()
        t.step(np.arange(40, dtype=np.int32), 0.2, 1, 1, 0.7, 1e-3, 0.9, 1e-7, frozen_mask)
        after_t, after_a = t.get_weights(), t.get_accumulators()
    finally:
        t.close()
    for layer, block in enumerate(blocks(13, units)):
        if (frozen_mask >> layer) & 1:
            assert np.array_equal(bits(before_t[block]), bits(after_t[block])), layer
            assert np.array_equal(bits(before_a[block]), bits(after_a[block])), layer
        else:
            assert np.all(after_a[block] != before_a[block]) and np.all(after_t[block] != before_t[block]), layer


@pytest.mark.parametrize('freeze_till', [0, 1, 2, 3])
def test_freeze_till_through_trainer(freeze_till):
    from mycroft_precise_amd.train import Trainer
    units = (40, 24)
    x, y = tt.learning_task(40, 4)
    tr = Trainer(weights=stacked_weights(13, units), params=ModelParams(recurrent_units=units, dropout=0.2, freeze_till=freeze_till), seed=3)
    try:
        assert tr.frozen_mask == (1 << freeze_till) - 1 and tr.units == units
        before_t, before_a = tr._t.get_weights(), tr._t.get_accumulators()
        tr.fit(x, y, batch_size=17, epochs=2)
        after_t, after_a = tr._t.get_weights(), tr._t.get_accumulators()
    finally:
        tr.close()
    for layer, block in enumerate(blocks(13, units)):
        if layer < freeze_till:
            assert np.array_equal(bits(before_t[block]), bits(after_t[block])) and not after_a[block].any(), layer
        else:
            assert np.all(after_a[block] != 0) and np.all(after_t[block] != before_t[block]), layer


# ---- 5. resident-set entry points ------------------------------------------------------------------------------------------
def test_append_gives_what_the_host_fed_call_gives():
    w = stacked_weights(13, (40, 33))
    x, y = tt.learning_task(50, 6)
    whole, grown = _lib.HipTrainer(w, 29, 13, stacked=True), _lib.HipTrainer(w, 29, 13, stacked=True)
    try:
        whole.set_data(x, y)
        grown.set_data(x[:19], y[:19])
        grown.append(x[19:], y[19:])
        grown.append(x[:7], y[:7], validation=True)
        assert grown.n_samples() == 50 and grown.n_samples(True) == 7
        back = grown.get_data()
        assert np.array_equal(back[0], x) and np.array_equal(back[1], y)
        idx = np.random.default_rng(1).permutation(50)[:33].astype(np.int32)
        losses = [t.step(idx, 0.2, 4, 0, 0.7, 1e-3, 0.9, 1e-7, 0) for t in (whole, grown)]
        assert np.float32(losses[0]).view(np.uint32) == np.float32(losses[1]).view(np.uint32)
        assert np.array_equal(bits(whole.get_weights()), bits(grown.get_weights()))
        assert np.array_equal(bits(grown.evaluate_models(source='data')[2][0]), bits(whole.evaluate(x)[2]))
        assert np.array_equal(bits(grown.evaluate_models(source='validation')[2][0]), bits(whole.evaluate(x[:7])[2]))
    finally:
        whole.close()
        grown.close()


def test_fit_resident_on_a_subset_equals_fit_on_its_rows():
    from mycroft_precise_amd.train import Trainer
    units = (40, 33)
    w = stacked_weights(13, units)
    x, y = tt.learning_task(23, 5)
    ids = np.random.default_rng(17).permutation(23)[:17]
    ids[-1] = ids[0]
    a, b = (Trainer(weights=w, params=ModelParams(recurrent_units=units, dropout=0.2), seed=9) for _ in range(2))
    try:
        a.set_data(x, y)
        ha = a.fit_resident(batch_size=5, epochs=2, shuffle=True, subset=ids)
        hb = b.fit(x[ids], y[ids], batch_size=5, epochs=2, shuffle=True)
        assert ha == hb and len(ha['loss']) == 2
        assert np.array_equal(bits(a._t.get_weights()), bits(b._t.get_weights()))
        assert np.array_equal(bits(a._t.get_accumulators()), bits(b._t.get_accumulators()))
        assert np.any(a._t.get_weights() != flatten_weights(w))
    finally:
        a.close()
        b.close()


def test_sample_choose_equals_the_host_rule():
    """the failing rows, (p > 0.5) != (y > 0.5) as precise-train-sampled counts them, by largest float32 error, from the
    trainer's own probabilities"""
    w = stacked_weights(13, (40, 33))
    x, y = tt.learning_task(90, 8)
    t = _lib.HipTrainer(w, 29, 13, stacked=True)
    try:
        t.set_data(x, y)
        probs = t.evaluate(x)[2]
        report, added, got_probs = t.sample_choose(7, 'error', want_probs=True)
        assert np.array_equal(bits(got_probs), bits(probs))
        err = np.abs(probs - y)
        failed = np.flatnonzero((probs > 0.5) != (y > 0.5))
        assert report['n'] == 90 and report['n_failed'] == failed.size and 7 <= failed.size
        order = failed[np.lexsort((failed, -err[failed]))]
        assert list(added) == list(order[:7]) and report['n_added'] == 7
        assert list(t.sample_selected()) == list(order[:7])
    finally:
        t.close()


def test_stats_over_the_trainers_own_probabilities():
    import test_stats as ts
    n = 257
    models = [stacked_weights(13, (64, 40), seed=31), stacked_weights(13, (20,), seed=32), stacked_weights(13, (20, 20), seed=33)]
    x = np.random.default_rng(n).normal(0.0, 3.0, (n, 29, 13)).astype(np.float32)
    y = ts.targets_for(n, n, fractional=False)
    t = _lib.HipTrainer(models, 29, 13, stacked=True)
    try:
        t.set_validation(x, y)
        want = t.evaluate_models(source='validation')[2]
        thr = np.sort(np.concatenate([np.linspace(0.0, 1.0, 90), [float(v) for v in want.reshape(-1)[:8]]]))
        for compare in ('f32', 'f64'):
            counts, summary, probs = t.stats_models(thresholds=thr, compare=compare, source='validation', want_probs=True)
            assert probs.tobytes() == want.tobytes()
            ts.assert_counts(counts, want, y, thr, compare)
            ts.assert_summary_ints(summary, want, y)
    finally:
        t.close()


def test_group_of_mixed_depths():
    """TrainerGroup over one- and two-layer candidates: .weights, .best, .stats; each candidate the bits of its own Trainer"""
    from mycroft_precise_amd.train import Trainer, TrainerGroup
    x, y = tt.learning_task(60, 1)
    xv, yv = tt.learning_task(30, 2)
    cands = [ModelParams(recurrent_units=20, freeze_till=0), ModelParams(recurrent_units=(24, 16), freeze_till=2, loss_bias=0.4),
             ModelParams(recurrent_units=(40, 33), dropout=0.3)]
    group = TrainerGroup(cands, seeds=(5, 6, 7))
    singles = [Trainer(params=p, seed=s) for p, s in zip(cands, (5, 6, 7))]
    try:
        assert group.units == [20, (24, 16), (40, 33)] and group.frozen_masks == [0, 3, 0]
        group.fit(x, y, batch_size=25, epochs=2, validation_data=(xv, yv), shuffle=False)
        weights = group.weights
        assert [len(w['gru']) for w in weights] == [1, 2, 2]
        for m, tr in enumerate(singles):
            tr.fit(x, y, batch_size=25, epochs=2, validation_data=(xv, yv), shuffle=False)
            assert np.array_equal(bits(flatten_weights(weights[m])), bits(tr._t.get_weights())), m
        assert group.best('val_loss') == int(np.argmin([h['val_loss'][-1] for h in group.histories]))
        sweeps = group.stats((0.5,), validation=True)
        assert len(sweeps) == 3
    finally:
        group.close()
        for tr in singles:
            tr.close()


def test_trial_reports_of_a_group_with_a_stacked_candidate():
    """test_train_wide.test_trial_reports_of_a_mixed_width_group over (20, (40, 33), 20): one multi-model runner per distinct
    ``units`` entry, the stacked candidate's holding its two-layer weights"""
    import math
    import test_stats as ts
    from mycroft_precise_amd import params as P
    from mycroft_precise_amd import stats as S
    from mycroft_precise_amd.network_runner import HipRunner
    from mycroft_precise_amd.train import TrainerGroup, trial_reports
    keep = dict(P.pr.__dict__)
    x, y = tt.learning_task(120, 1)
    xv, yv = tt.learning_task(70, 2)
    group = TrainerGroup([ModelParams(recurrent_units=u, loss_bias=b) for u, b in ((20, 0.7), ((40, 33), 0.7), (20, 0.4))], seeds=(5, 6, 7))
    runners = []
    try:
        group.fit(x, y, batch_size=40, epochs=2, validation_data=(xv, yv))
        noise = [synth.stream_pcm(900 + i, n).astype(np.float32) / np.float32(32768.0) for i, n in enumerate((40000, 61234))]
        weights = group.weights
        runners = [HipRunner(weights=[weights[0], weights[2]]), HipRunner(weights=[weights[1]])]
        reports = trial_reports(group, runners, noise, interaction_estimate=100, ambient_annoyance=1.0)
        pred = group.predict(xv)
        windows = {0: (runners[0], 0), 2: (runners[0], 1), 1: (runners[1], 0)}
        seconds = 0.0
        for a in noise:
            seconds += len(a) / P.pr.sample_rate
        for m, report in enumerate(reports):
            runner, slot = windows[m]
            per_recording = [w[slot] for w in runner.evaluate_clips(noise, 4096)]
            assert report['test_stats'] == S.Stats(pred[m], yv.reshape(-1, 1), []).to_dict()
            annoyance, ww, nww, threshold, _ = ts.ref.estimate(pred[m][yv > 0.5], per_recording, seconds, 100, 1.0)
            size = 1.0 + math.exp((group._t.n_params[m] - 11000) / 10000)
            assert report['best_threshold'] == threshold
            assert report['cost_info'] == {'params_cost': size, 'annoyance': annoyance, 'ww_annoyance': ww, 'nww_annoyance': nww}
        assert group.best('cost') == int(np.argmin([r['cost'] for r in reports]))
    finally:
        for r in runners:
            r.engine.close()
        group.close()
        P.pr.__dict__.clear()
        P.pr.__dict__.update(keep)


# ---- 6. serving round trip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('units', [(64, 64), (256, 256)])
def test_trained_stacked_model_is_served(tmp_path, units):
    """Trainer.save -> HipRunner.predict in float32 within test_train_wide's round-trip bounds; a gru_precision='bf16' engine
    loads the same file and stays inside the bf16 contract's two-tier tolerance (test_bf16_wide.check)"""
    import test_bf16_wide as tb
    from mycroft_precise_amd.network_runner import HipRunner
    from mycroft_precise_amd.train import Trainer
    x, y = tt.learning_task(64, 3)
    tr = Trainer(params=ModelParams(recurrent_units=units, dropout=0.2), seed=1)
    try:
        start = tr._t.get_weights()
        tr.fit(x, y, batch_size=32, epochs=2)
        path = str(tmp_path / 'trained.npz')
        tr.save(path)
        got_trainer = tr.predict(x)
        # every layer moved (not "every parameter": of 600 k parameters that each move by about +-3e-3 four times, one or two
        # land on the float32 they started from)
        moved = tr._t.get_weights() != start
        print('%s: %d of %d parameters differ from the initial network' % (units, moved.sum(), moved.size))
        assert all(moved[block].mean() >= 0.9999 for block in blocks(13, units))
    finally:
        tr.close()
    loaded = load_weights(path)
    assert [layer[1].shape for layer in loaded['gru']] == [(units[0], 3 * units[0]), (units[1], 3 * units[1])]
    want = ref.forward_numpy(loaded, x)['p'].reshape(-1, 1)
    runner = HipRunner(path)
    got_engine = runner.predict(x)
    runner.engine.close()
    d_trainer, d_engine = float(np.abs(got_trainer - want).max()), float(np.abs(got_engine - want).max())
    print('%s: Trainer.predict %.3g, HipRunner.predict %.3g from float64' % (units, d_trainer, d_engine))
    assert d_trainer <= PROB_TOL
    assert d_engine <= 1e-4
    eng = tb.engine(loaded, 29)
    try:
        got_bf16 = eng.predict(x)[:, 0]
    finally:
        eng.close()
    tb.check('trained %dx%d' % units, got_bf16, x, loaded, public=True)


# ---- 7. learning -----------------------------------------------------------------------------------------------------------
def reference_training(weights, x, y, xv, yv, batch, epochs, rate, loss_bias, seed):
    """test_train.reference_training for a stacked network: float64 on the CPU, the same masks of both layers, torch autograd,
    the RMSprop formula"""
    import torch
    params = ref.tensors(weights)
    accum = [np.zeros(tuple(p.shape)) for p in params]
    H1 = weights['gru'][0][1].shape[0]
    step = 0
    for _ in range(epochs):
        for a in range(0, len(x), batch):
            xb, yb = x[a:a + batch], y[a:a + batch]
            masks = masks_for(seed, step, len(xb), x.shape[2], H1, rate)
            out = ref.forward(params, xb, masks)
            loss = ref.weighted_log_loss(out['p'], torch.as_tensor(np.asarray(yb, dtype=np.float64)), loss_bias)
            grads = torch.autograd.grad(loss, params)
            with torch.no_grad():
                for i, (p, g) in enumerate(zip(params, grads)):
                    new, accum[i] = ref.rmsprop(p.numpy(), accum[i], g.numpy())
                    p.copy_(torch.from_numpy(new))
            step += 1
    with torch.no_grad():
        out = ref.forward(params, xv, None)
        loss = ref.weighted_log_loss(out['p'], torch.as_tensor(np.asarray(yv, dtype=np.float64)), loss_bias)
    return float(loss), float(np.mean(np.rint(out['p'].numpy()) == yv))


def test_training_learns_like_the_reference_trainer():
    """test_train.test_training_learns_like_the_reference_trainer on a (48, 33) network, with that test's bounds"""
    from mycroft_precise_amd.train import Trainer
    x, y = tt.learning_task(512, 1)
    xv, yv = tt.learning_task(256, 2)
    weights = synth.make_weights(13, (48, 33), seed=5)
    tr = Trainer(weights=weights, params=ModelParams(recurrent_units=(48, 33), dropout=0.2, loss_bias=0.7), seed=17)
    try:
        start = tr.evaluate(xv, yv)[0]
        hist = tr.fit(x, y, batch_size=128, epochs=30, validation_data=(xv, yv), shuffle=False)
    finally:
        tr.close()
    want_loss, want_acc = reference_training(weights, x, y, xv, yv, 128, 30, 0.2, 0.7, 17)
    got_loss, got_acc = hist['val_loss'][-1], hist['val_acc'][-1]
    print('validation loss %.4f -> %.5f (reference trainer %.5f, difference %.2f %%), accuracy %.4f (reference %.4f)' %
          (start, got_loss, want_loss, 100 * abs(got_loss - want_loss) / want_loss, got_acc, want_acc))
    assert len(hist['loss']) == 30 and hist['loss'][-1] < hist['loss'][0]
    assert got_loss <= 0.05
    assert got_acc >= 0.97
    assert abs(got_loss - want_loss) <= 0.05 * want_loss


# ---- 8. argument errors ----------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched():
    ptr = tt.ptr
    lib = _lib.load()
    t = _lib.HipTrainer(stacked_weights(13, (40, 33)), 29, 13, stacked=True)
    x = tt.candidates('n01', 4)
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

    try:
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
        with pytest.raises(ValueError, match='stacked network takes masks'):
            t.loss_grad(x, y, masks=_lib.dropout_masks(0, 0, 4, 13, 0.2))
        with pytest.raises(ValueError, match=r'masks must be \[3, 4, 40\]'):
            t.loss_grad(x, y, masks=(_lib.dropout_masks(0, 0, 4, 13, 0.2), _lib.dropout_masks(0, 0, 4, 33, 0.2, layer=1)))
    finally:
        t.close()
