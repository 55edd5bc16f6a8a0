"""GPU: the training kernels (csrc/gru_train_device.h) against the float64 autograd reference of train_reference.py.

Bounds: gradients per tensor max|d| / max|reference tensor| <= 1e-5 (about 20x the float32 floor, which is
torch float32 autograd against the same float64 reference: 0.4e-7 .. 5.4e-7), loss <= 1e-6, probabilities <= 1e-5.  All
batches are built from kink-safe candidates only (train_reference.kink_safe): every hard-sigmoid pre-activation at least
1e-3 from +-2.5 and |logit| <= 8 in the float64 reference, and every test asserts that at least half its candidates pass.
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
