"""GPU: training of 33..256-unit networks (pe_trainer_create_wide, csrc/gru_train_wide_device.h) against the
float64 autograd reference of train_reference.py, and the bit-level properties of the wide path.

Bounds: the ones of test_train.py, GRAD_TOL = 1e-5, LOSS_TOL = 1e-6, PROB_TOL = 1e-5: 20x the float32 floor, which is torch
float32 autograd against the same float64 reference (train_reference.loss_and_grads(dtype=float32), measured on the CPU):
  gradients  H in {33, 48, 64, 96, 120, 128, 256}, F = 13, T in {3, 29}: 2.6e-7 .. 4.9e-7;  H = 256, F = 32, T = 64: 5.2e-7;
             H = 128, F = 26, T = 29: 2.7e-7 -- all inside the 0.4e-7 .. 5.4e-7 band the bounds were derived from;
  loss <= 4.2e-8, probabilities <= 7.6e-8.
Every batch is built from kink-safe candidates (test_train.safe_batch: at least half of the candidates must pass, which the
float64 reference alone decides).  'n01' inputs never saturate a gate at these widths, so the 'n03', T = 3 cases carry the
zero-derivative side of the hard sigmoid: each of them asserts that the kept samples hold saturated and unsaturated gates.
The sample tile of the wide kernels is 16, as it is for the narrow ones.
"""
import functools

import numpy as np
import pytest

import test_train as tt
import train_reference as ref
from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.model import ModelParams, load_weights

pytestmark = pytest.mark.gpu

TILE = 16
N03_WIDTHS = (33, 40, 64, 100, 128, 192, 256)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def wide_weights(F, H, seed=0):
    return synth.make_weights(F, (H,)) if seed == 0 else synth.make_weights(F, (H,), seed=seed)


@pytest.fixture
def wide(monkeypatch):
    """test_train's helpers make their trainers through _lib.HipTrainer: here with wide=True"""
    monkeypatch.setattr(_lib, 'HipTrainer', functools.partial(_lib.HipTrainer, wide=True))


@functools.lru_cache(maxsize=None)
def n03_pool(H):
    """the 'n03', rate 0.2, T = 3 row of the issue: up to 33 kink-safe samples of 256 candidates, seed H + 3"""
    w = wide_weights(13, H)
    x, masks = tt.safe_batch(w, 'n03', 33, 256, T=3, F=13, rate=0.2, seed=H + 3)
    out = ref.forward_numpy(w, x, masks)
    a = np.abs(np.concatenate([out['a_z'], out['a_r']], axis=2))
    assert (a > 2.5).any() and (a < 2.5).any()            # both sides of the hard sigmoid's kinks
    return w, x, masks


# ---- 1. gradients, loss and probabilities against float64 ----------------------------------------------------------------
@pytest.mark.parametrize('n', [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
@pytest.mark.parametrize('H', N03_WIDTHS)
def test_gradients_every_width_and_tile_edge(wide, H, n):
    w, x, masks = n03_pool(H)
    tt.check_against_reference(w, x[:n], tt.targets_for(n, H), masks[:, :n], T=3)


@pytest.mark.parametrize('T', [1, 2, 29])
@pytest.mark.parametrize('H', [33, 128])
def test_gradients_chain_lengths(wide, H, T):
    w = wide_weights(13, H)
    x, _ = tt.safe_batch(w, 'n01', 33, 256, T=T, F=13, seed=H + T)
    tt.check_against_reference(w, x, tt.targets_for(33, T), T=T)


@pytest.mark.parametrize('T,F,H,seed', [(64, 32, 256, 5), (29, 26, 128, 7), (29, 1, 33, 9)])
def test_gradients_shapes(wide, T, F, H, seed):
    w = wide_weights(F, H)
    x, masks = tt.safe_batch(w, 'n01', 33, 256, T=T, F=F, rate=0.2, seed=seed)
    tt.check_against_reference(w, x, tt.targets_for(33, T), masks, T=T)


def test_gradients_saturating_long_chain(wide):
    w = wide_weights(13, 128)
    x, _ = tt.safe_batch(w, 'n03', 33, 256, T=29, F=13, seed=170)
    tt.check_against_reference(w, x, tt.targets_for(33, 170))


@pytest.mark.parametrize('loss_bias', [0.0, 0.7, 1.0])
def test_gradients_loss_bias(wide, loss_bias):
    w, x, masks = n03_pool(64)
    tt.check_against_reference(w, x, tt.targets_for(33, 5), masks, loss_bias=loss_bias, T=3)


@pytest.mark.parametrize('target', [0.0, 1.0])
def test_gradients_constant_targets(wide, target):
    w, x, masks = n03_pool(64)
    tt.check_against_reference(w, x, np.full(33, target, dtype=np.float32), masks, T=3)


def test_gradients_more_tiles_than_compute_units(wide):
    """258 tiles for 256 compute units, the last tile one sample; 64 gradient chunks of 116 or 117 records"""
    n = 257 * TILE + 1
    w = wide_weights(13, 64)
    x, _ = tt.safe_batch(w, 'n01', n, 4400, seed=11)
    tt.check_against_reference(w, x, tt.targets_for(n, 11))


# ---- 2. padding is inert ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [33, 100])
def test_stale_scratch_is_never_read(H):
    """A short call after a larger call with larger values on the same trainer: tape, D, partials and chunk partials then hold
    what the larger call left; the result is the fresh trainer's in bits."""
    w = wide_weights(13, H)
    big = tt.candidates('n03', 80, seed=H) * np.float32(10.0)
    small = tt.candidates('n01', TILE + 1, seed=H + 1)
    y_big, y_small = tt.targets_for(80, 1), tt.targets_for(TILE + 1, 2)
    masks = _lib.dropout_masks(3, 0, TILE + 1, 13, 0.2)
    idx_big, idx_small = np.arange(80, dtype=np.int32), np.arange(80, 80 + TILE + 1, dtype=np.int32)
    used, fresh = _lib.HipTrainer(w, 29, 13, wide=True), _lib.HipTrainer(w, 29, 13, wide=True)
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


# ---- 3. bit-level properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [33, 240])
@pytest.mark.parametrize('H', [40, 128])
def test_step_is_gradient_then_apply_and_repeats(H, n):
    w = wide_weights(13, H)
    rng = np.random.default_rng(n + H)
    data, labels = tt.candidates('n03', 300, seed=21), tt.targets_for(300, 21)
    idx = rng.permutation(300)[:n].astype(np.int32)
    seed, step, rate = 99, 5, 0.2
    fused, again, manual = (_lib.HipTrainer(w, 29, 13, wide=True) for _ in range(3))
    try:
        fused.set_data(data, labels)
        again.set_data(data, labels)
        for k in range(2):                      # two steps: the second starts from non-zero accumulators
            loss_f = fused.step(idx, rate, seed, step + k, 0.7, 1e-3, 0.9, 1e-7, 0)
            loss_a = again.step(idx, rate, seed, step + k, 0.7, 1e-3, 0.9, 1e-7, 0)
            masks = _lib.dropout_masks(seed, step + k, n, 13, rate)
            loss_m, grads, probs = manual.loss_grad(data[idx], labels[idx], masks=masks, loss_bias=0.7)
            loss_m2, grads2, probs2 = manual.loss_grad(data[idx], labels[idx], masks=masks, loss_bias=0.7)
            assert loss_m == loss_m2 and np.array_equal(bits(grads), bits(grads2)) and np.array_equal(bits(probs), bits(probs2))
            manual.apply(grads, 1e-3, 0.9, 1e-7, 0)
            for other, loss_o in ((again, loss_a), (manual, loss_m)):
                assert np.float32(loss_f).view(np.uint32) == np.float32(loss_o).view(np.uint32)
                assert np.array_equal(bits(fused.get_weights()), bits(other.get_weights()))
                assert np.array_equal(bits(fused.get_accumulators()), bits(other.get_accumulators()))
        assert fused.get_accumulators().all() and not np.array_equal(fused.get_weights(), synth_flat(w))
    finally:
        for t in (fused, again, manual):
            t.close()


def synth_flat(w):
    from mycroft_precise_amd.train import flatten_weights
    return flatten_weights(w)


GROUP_WIDTHS = (8, 20, 40, 128, 20)


@pytest.mark.parametrize('n', [33, 240])
def test_alone_equals_together_in_a_mixed_group(n):
    """each network of a (narrow, narrow, wide, wide, narrow) trainer against a trainer of its own; the narrow ones also
    against pe_trainer_create[_models] trainers; then the same group in another order"""
    models = [wide_weights(13, h, seed=10 + i) for i, h in enumerate(GROUP_WIDTHS)]
    data, labels = tt.candidates('n03', 300, seed=22), tt.targets_for(300, 22)
    idx = np.random.default_rng(n).permutation(300)[:n].astype(np.int32)
    hp = dict(dropout_rate=(0.2, 0.0, 0.2, 0.2, 0.3), seed=(7, 8, 9, 10, 11), loss_bias=(0.3, 0.7, 0.7, 0.5, 0.9),
              lr=(1e-3, 2e-3, 1e-3, 5e-4, 1e-3))

    def alone(m, wide):
        t = _lib.HipTrainer(models[m], 29, 13, wide=wide)
        t.set_data(data, labels)
        losses = [np.float32(t.step(idx, hp['dropout_rate'][m], hp['seed'][m], 4 + k, hp['loss_bias'][m], hp['lr'][m], 0.9, 1e-7, 0))
                  for k in range(2)]
        out = (losses, t.get_weights(), t.get_accumulators(), t.evaluate(data[:n])[2])
        t.close()
        return out

    def together(order):
        g = _lib.HipTrainer([models[m] for m in order], 29, 13, wide=True)
        g.set_data(data, labels)
        sub = {k: tuple(v[m] for m in order) for k, v in hp.items()}
        losses = [g.step_models(idx, step=4 + k, rho=0.9, eps=1e-7, **sub) for k in range(2)]
        out = (losses, g.split(g.get_weights()), g.split(g.get_accumulators()), g.evaluate_models(data[:n])[2])
        g.close()
        return out

    singles = [alone(m, True) for m in range(len(models))]
    for order in ((0, 1, 2, 3, 4), (3, 4, 0, 2, 1)):
        losses, theta, accum, probs = together(order)
        for pos, m in enumerate(order):
            want = singles[m]
            for k in range(2):
                assert np.float32(losses[k][pos]).view(np.uint32) == want[0][k].view(np.uint32), (order, m, k)
            assert np.array_equal(bits(theta[pos]), bits(want[1])), (order, m)
            assert np.array_equal(bits(accum[pos]), bits(want[2])), (order, m)
            assert np.array_equal(bits(probs[pos]), bits(want[3])), (order, m)
    for m, h in enumerate(GROUP_WIDTHS):
        if h <= 32:
            narrow = alone(m, False)
            assert [v.view(np.uint32) for v in narrow[0]] == [v.view(np.uint32) for v in singles[m][0]]
            for a, b in zip(narrow[1:], singles[m][1:]):
                assert np.array_equal(bits(a), bits(b)), m


@pytest.mark.parametrize('H', [40, 128])
def test_one_forward(H):
    n = 240
    w = wide_weights(13, H)
    x, y = tt.candidates('n03', n, seed=23), tt.targets_for(n, 23)
    rows = np.random.default_rng(H).permutation(n).astype(np.int32)
    t = _lib.HipTrainer([w], 29, 13, wide=True)
    try:
        t.set_data(x, y)
        t.set_validation(x[::-1], y[::-1])
        want = t.evaluate_models(x, y)[2][0]
        assert np.array_equal(bits(t.evaluate_models(source='data')[2][0]), bits(want))
        assert np.array_equal(bits(t.evaluate_models(source='validation')[2][0]), bits(want[::-1]))
        assert np.array_equal(bits(t.evaluate_indices(rows)[2][0]), bits(want[rows]))
        assert np.array_equal(bits(t.stats_models(thresholds=(0.5,), source='data', want_probs=True)[2][0]), bits(want))
        assert np.array_equal(bits(t.stats_models(x, y, thresholds=(0.5,), source='host', want_probs=True)[2][0]), bits(want))
        assert np.array_equal(bits(t.sample_choose(5, 'error', want_probs=True)[2]), bits(want))
        assert np.array_equal(bits(t.evaluate_models(x, y)[2][0]), bits(want))
    finally:
        t.close()
    assert float(np.abs(want - ref.forward_numpy(w, x)['p']).max()) <= tt.PROB_TOL


# ---- 4. frozen layers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('freeze_till', [1, 2])
def test_frozen_layers_keep_their_bits(freeze_till):
    from mycroft_precise_amd.train import Trainer
    w = wide_weights(13, 64)
    n_gru = (13 + 64 + 1) * 192
    x, y = tt.learning_task(40, 4)
    tr = Trainer(weights=w, params=ModelParams(recurrent_units=64, dropout=0.2, freeze_till=freeze_till), seed=3)
    try:
        before_t, before_a = tr._t.get_weights(), tr._t.get_accumulators()
        tr.fit(x, y, batch_size=17, epochs=2)
        after_t, after_a = tr._t.get_weights(), tr._t.get_accumulators()
    finally:
        tr.close()
    frozen = slice(0, n_gru) if freeze_till == 1 else slice(0, before_t.size)
    assert np.array_equal(bits(before_t[frozen]), bits(after_t[frozen]))
    assert np.array_equal(bits(before_a[frozen]), bits(after_a[frozen]))
    if freeze_till == 1:
        assert np.all(after_a[n_gru:] != before_a[n_gru:]) and np.all(after_t[n_gru:] != before_t[n_gru:])


def test_unfrozen_everything_moves():
    w = wide_weights(13, 64)
    x, y = tt.learning_task(40, 4)
    t = _lib.HipTrainer(w, 29, 13, wide=True)
    try:
        before = t.get_weights()
        t.set_data(x, y)
        t.step(np.arange(40, dtype=np.int32), 0.2, 1, 0, 0.7, 1e-3, 0.9, 1e-7, 0)
        assert np.all(t.get_accumulators() != 0) and np.all(t.get_weights() != before)
    finally:
        t.close()


# ---- 5. resident-set entry points ------------------------------------------------------------------------------------------
def test_fit_resident_on_a_subset_equals_fit_on_its_rows():
    from mycroft_precise_amd.train import Trainer
    w = wide_weights(13, 64)
    x, y = tt.learning_task(23, 5)
    ids = np.random.default_rng(17).permutation(23)[:17]
    ids[-1] = ids[0]
    a, b = (Trainer(weights=w, params=ModelParams(recurrent_units=64, dropout=0.2), seed=9) for _ in range(2))
    try:
        a.set_data(x, y)
        ha = a.fit_resident(batch_size=5, epochs=2, shuffle=True, subset=ids)
        hb = b.fit(x[ids], y[ids], batch_size=5, epochs=2, shuffle=True)
        assert ha == hb and len(ha['loss']) == 2
        assert np.array_equal(bits(a._t.get_weights()), bits(b._t.get_weights()))
        assert np.array_equal(bits(a._t.get_accumulators()), bits(b._t.get_accumulators()))
        assert np.any(a._t.get_weights() != synth_flat(w))
    finally:
        a.close()
        b.close()


def test_stats_over_the_trainers_own_probabilities():
    import test_stats as ts
    n = 257
    models = [wide_weights(13, 64, seed=31), wide_weights(13, 20, seed=32)]
    x = np.random.default_rng(n).normal(0.0, 3.0, (n, 29, 13)).astype(np.float32)
    y = ts.targets_for(n, n, fractional=False)
    t = _lib.HipTrainer(models, 29, 13, wide=True)
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


def test_sampled_trainer_equals_the_scripts_loop(tmp_path):
    import test_sampled as tsm
    from mycroft_precise_amd.train import Trainer
    rng = np.random.default_rng(12)
    x = rng.normal(0.0, 1.0, (40, 29, 13))
    y = (rng.random((40, 1)) < 0.5).astype(np.float64)
    x, y = tsm.duplicated(x, y, [(1, 39), (5, 6)])
    w = wide_weights(13, 64)
    tsm.run_both(lambda: Trainer(w, ModelParams(recurrent_units=64), seed=7), x, y, 'error', tmp_path, cycles=2, epochs=1)


def test_trial_reports_of_a_mixed_width_group():
    """test_stats.test_trial_reports_equal_the_host_loop over widths (20, 64, 20): one multi-model runner per width"""
    import math
    import test_stats as ts
    from mycroft_precise_amd import params as P
    from mycroft_precise_amd import stats as S
    from mycroft_precise_amd.network_runner import HipRunner
    from mycroft_precise_amd.train import TrainerGroup, trial_reports
    keep = dict(P.pr.__dict__)
    x, y = tt.learning_task(120, 1)
    xv, yv = tt.learning_task(70, 2)
    group = TrainerGroup([ModelParams(recurrent_units=u, loss_bias=b) for u, b in ((20, 0.7), (64, 0.7), (20, 0.4))], seeds=(5, 6, 7))
    runners = []
    try:
        group.fit(x, y, batch_size=40, epochs=2, validation_data=(xv, yv))
        noise = [synth.stream_pcm(900 + i, n).astype(np.float32) / np.float32(32768.0) for i, n in enumerate((40000, 61234))]
        weights = group.weights
        runners = [HipRunner(weights=[weights[0], weights[2]]), HipRunner(weights=[weights[1]])]
        with pytest.raises(ValueError, match='one width'):
            trial_reports(group, runners[0], noise)
        with pytest.raises(ValueError, match='2 widths'):
            trial_reports(group, runners[:1], noise)
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
        assert group.best('val_loss') == int(np.argmin([h['val_loss'][-1] for h in group.histories]))
    finally:
        for r in runners:
            r.engine.close()
        group.close()
        P.pr.__dict__.clear()
        P.pr.__dict__.update(keep)


# ---- 6. serving round trip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [64, 256])
def test_trained_wide_model_is_served(tmp_path, H):
    from mycroft_precise_amd.network_runner import HipRunner
    from mycroft_precise_amd.train import Trainer
    x, y = tt.learning_task(64, 3)
    tr = Trainer(params=ModelParams(recurrent_units=H, dropout=0.2), seed=1)
    try:
        start = tr._t.get_weights()
        tr.fit(x, y, batch_size=32, epochs=2)
        path = str(tmp_path / 'trained.npz')
        tr.save(path)
        got_trainer = tr.predict(x)
        assert np.all(tr._t.get_weights() != start)
    finally:
        tr.close()
    loaded = load_weights(path)
    assert loaded['gru'][0][1].shape == (H, 3 * H)
    want = ref.forward_numpy(loaded, x)['p'].reshape(-1, 1)
    got_engine = HipRunner(path).predict(x)
    d_trainer, d_engine = float(np.abs(got_trainer - want).max()), float(np.abs(got_engine - want).max())
    print('H=%d: Trainer.predict %.3g, HipRunner.predict %.3g from float64' % (H, d_trainer, d_engine))
    assert d_trainer <= tt.PROB_TOL
    assert d_engine <= 1e-4


# ---- 7. learning -----------------------------------------------------------------------------------------------------------
def test_training_learns_like_the_reference_trainer():
    """test_train.test_training_learns_like_the_reference_trainer at recurrent_units = 64, with that test's bounds"""
    from mycroft_precise_amd.train import Trainer
    x, y = tt.learning_task(512, 1)
    xv, yv = tt.learning_task(256, 2)
    weights = synth.make_weights(13, (64,), seed=5)
    tr = Trainer(weights=weights, params=ModelParams(recurrent_units=64, dropout=0.2, loss_bias=0.7), seed=17)
    try:
        start = tr.evaluate(xv, yv)[0]
        hist = tr.fit(x, y, batch_size=128, epochs=30, validation_data=(xv, yv), shuffle=False)
    finally:
        tr.close()
    want_loss, want_acc = tt.reference_training(weights, x, y, xv, yv, 128, 30, 0.2, 0.7, 17)
    got_loss, got_acc = hist['val_loss'][-1], hist['val_acc'][-1]
    print('validation loss %.4f -> %.5f (reference trainer %.5f, difference %.2f %%), accuracy %.4f (reference %.4f)' %
          (start, got_loss, want_loss, 100 * abs(got_loss - want_loss) / want_loss, got_acc, want_acc))
    assert len(hist['loss']) == 30 and hist['loss'][-1] < hist['loss'][0]
    assert got_loss <= 0.05
    assert got_acc >= 0.97
    assert abs(got_loss - want_loss) <= 0.05 * want_loss
