"""GPU: several networks trained in one launch (pe_trainer_create_models / pe_trainer_step_models / pe_trainer_evaluate_models,
``train.TrainerGroup``) against the same networks in trainers of their own.

The bound is equality of bits (float32 compared as uint32 views, Python floats with ==): a network's sums run in an order that
depends neither on the width of the launch nor on the other networks in it ("Several networks"), and the
single trainer is held to the float64 reference by test_train.py."""
import functools

import numpy as np
import pytest

from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.model import ModelParams, load_weights

pytestmark = pytest.mark.gpu

LR, RHO, EPS = 1e-3, 0.9, 1e-7


def candidates(family, n, T=29, F=13, seed=0):           # (test_train.py's; only the normal families are used here)
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 3.0 if family == 'n03' else 1.0, (n, T, F)).astype(np.float32)


def targets_for(n, seed=0):
    return (np.random.default_rng(100 + seed).random(n) < 0.5).astype(np.float32)


def learning_task(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (n, 29, 13)).astype(np.float32)
    y = (rng.random(n) < 0.5).astype(np.float32)
    x[y > 0, 12:20, 2:5] += np.float32(1.5)
    return x, y


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def dataset(T=29, F=13):
    return candidates('n03', 300, T, F, seed=21), targets_for(300, 21)


# the four networks of the stock-shape case: widths 1 / 20 / 20 / 32 -> 64 / 320 / 320 / 512 threads in a launch of 512
WIDTHS = (1, 20, 20, 32)
HP = dict(dropout_rate=(0.0, 0.2, 0.5, 0.2), seed=(7, 7, 8, 9), loss_bias=(0.7, 0.3, 1.0, 0.0), frozen_mask=(0, 1, 2, 0),
          lr=(1e-3, 1e-3, 3e-3, 1e-3))


def make_models(widths, F=13):
    return [synth.make_weights(F, (h,), seed=10 + i) for i, h in enumerate(widths)]


def batches(counts, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.permutation(300)[:n].astype(np.int32) for n in counts]


@functools.lru_cache(maxsize=None)
def alone(widths, T, F, counts):
    """every network stepped in a HipTrainer of its own -> per network a list over steps of (loss, weights, accumulators);
    computed once per case and shared"""
    x, y = dataset(T, F)
    out = []
    for m, w in enumerate(make_models(widths, F)):
        t = _lib.HipTrainer(w, T, F)
        t.set_data(x, y)
        steps = []
        for k, idx in enumerate(batches(counts)):
            hp = {name: v[m] for name, v in hparams_for(widths).items()}
            loss = t.step(idx, hp['dropout_rate'], hp['seed'], 3 + k, hp['loss_bias'], hp['lr'], RHO, EPS, hp['frozen_mask'])
            steps.append((np.float32(loss), t.get_weights(), t.get_accumulators()))
        t.close()
        out.append(steps)
    return out


def hparams_for(widths):
    return {name: tuple(v[:len(widths)]) for name, v in HP.items()}


def run_group(widths, T, F, counts, order):
    """the same networks in ONE trainer, in the given model order -> the same structure as alone(), in the ORIGINAL order"""
    x, y = dataset(T, F)
    models = make_models(widths, F)
    hp = hparams_for(widths)
    g = _lib.HipTrainer([models[m] for m in order], T, F)
    assert g.n_models == len(order) and g.units == [widths[m] for m in order]
    assert g.n_params == [(F + widths[m] + 1) * 3 * widths[m] + widths[m] + 1 for m in order] and sum(g.n_params) == g.n_params_total
    g.set_data(x, y)
    out = [[] for _ in widths]
    for k, idx in enumerate(batches(counts)):
        loss = g.step_models(idx, step=3 + k, rho=RHO, eps=EPS, **{name: [v[m] for m in order] for name, v in hp.items()})
        theta, accum = g.split(g.get_weights()), g.split(g.get_accumulators())
        for pos, m in enumerate(order):
            out[m].append((loss[pos], theta[pos].copy(), accum[pos].copy()))
    g.close()
    return out


def assert_same_runs(got, want):
    for m, (g_steps, w_steps) in enumerate(zip(got, want)):
        assert len(g_steps) == len(w_steps)
        for k, ((gl, gt, ga), (wl, wt, wa)) in enumerate(zip(g_steps, w_steps)):
            assert same_bits(gl, wl), 'loss of model %d, step %d: %r != %r' % (m, k, gl, wl)
            assert same_bits(gt, wt), 'parameters of model %d, step %d' % (m, k)
            assert same_bits(ga, wa), 'accumulators of model %d, step %d' % (m, k)


STOCK_CASE = (WIDTHS, 29, 13, (33, 33, 16))          # three tiles, the last with one sample; then one full tile
BIG_LDS_CASE = ((3, 32), 64, 32, (17,))               # 78.7 KB of LDS (the > 48 KB opt-in) next to a narrow network


@pytest.mark.parametrize('case', [STOCK_CASE, BIG_LDS_CASE], ids=['29x13_w1-20-20-32', '64x32_w3-32'])
def test_alone_equals_together(case):
    widths, T, F, counts = case
    want = alone(widths, T, F, counts)
    assert all(step[2].any() for steps in want[:1] for step in steps)      # (the optimizer moved)
    assert_same_runs(run_group(widths, T, F, counts, list(range(len(widths)))), want)


def test_order_and_company_do_not_matter():
    widths, T, F, counts = STOCK_CASE
    want = alone(widths, T, F, counts)
    assert_same_runs(run_group(widths, T, F, counts, [3, 2, 1, 0]), want)
    # other company: the widest network leaves, the launch narrows to 320 threads
    got = run_group(widths[:3], T, F, counts, [1, 0, 2])
    assert_same_runs(got, want[:3])


def ptr(a):
    return None if a is None else a.ctypes.data


def test_group_of_one_is_the_single_trainer(stock_weights):
    lib = _lib.load()
    x, y = dataset()
    idx = batches((33, 16))
    single = _lib.HipTrainer(stock_weights, 29, 13)
    one = _lib.HipTrainer([stock_weights], 29, 13)
    by_step = _lib.HipTrainer([stock_weights], 29, 13)
    assert one.n_models == 1 and one.units == [20] and one.n_params == [single.n_params] and one.n_params_total == single.n_params
    for t in (single, one, by_step):
        t.set_data(x, y)
    for k, i in enumerate(idx):
        want = np.float32(single.step(i, 0.2, 99, k, 0.7, LR, RHO, EPS, 0))
        got = one.step_models(i, step=k, dropout_rate=0.2, seed=99, loss_bias=0.7, lr=LR, rho=RHO, eps=EPS, frozen_mask=0)
        loss = np.zeros(1, dtype=np.float32)              # pe_trainer_step on the trainer made by pe_trainer_create_models
        assert lib.pe_trainer_step(by_step._h, ptr(i), i.size, 0.2, 99, k, 0.7, LR, RHO, EPS, 0, ptr(loss)) == _lib.PE_OK
        for t, l in ((one, got[0]), (by_step, loss[0])):
            assert same_bits(l, want)
            assert same_bits(t.get_weights(), single.get_weights()) and same_bits(t.get_accumulators(), single.get_accumulators())
    for t in (single, one, by_step):
        t.close()


def test_resident_evaluation_is_the_host_evaluation():
    widths = WIDTHS
    models = make_models(widths)
    biases = list(HP['loss_bias'])
    x, y = dataset()
    g = _lib.HipTrainer(models, 29, 13)
    with pytest.raises(ValueError, match='validation'):                   # PE_ERR_INVALID: never set
        g.evaluate_models(source='validation', loss_bias=biases)
    with pytest.raises(ValueError, match='training'):
        g.evaluate_models(source='data', loss_bias=biases)
    lib = _lib.load()
    assert [lib.pe_trainer_n_samples(g._h, src) for src in (0, 1, 2)] == [-1, 0, 0]
    g.set_data(x[:33], y[:33])
    g.set_validation(x[40:41], y[40:41])
    assert [lib.pe_trainer_n_samples(g._h, src) for src in (1, 2)] == [33, 1]
    for source, sl in (('data', slice(0, 33)), ('validation', slice(40, 41))):
        n = sl.stop - sl.start
        res_loss, res_acc, res_probs = g.evaluate_models(source=source, loss_bias=biases)
        host_loss, host_acc, host_probs = g.evaluate_models(x[sl], y[sl], loss_bias=biases)
        none_loss, none_acc, pred = g.evaluate_models(x[sl])
        assert res_probs.shape == host_probs.shape == pred.shape == (4, n) and none_loss is None and none_acc is None
        for m, w in enumerate(models):
            t = _lib.HipTrainer(w, 29, 13)
            want_loss, want_acc, want_probs = t.evaluate(x[sl], y[sl], loss_bias=biases[m])
            t.close()
            assert want_acc == float(np.float32(np.mean(np.rint(want_probs) == y[sl])))
            for loss, acc, probs in ((res_loss, res_acc, res_probs), (host_loss, host_acc, host_probs)):
                assert float(acc[m]) == want_acc, (source, m)
                assert same_bits(loss[m], np.float32(want_loss)) and same_bits(probs[m], want_probs), (source, m)
            assert same_bits(pred[m], want_probs)
    # without the probabilities nothing but 2 K numbers comes back, and they are the same numbers
    loss2, acc2, none = g.evaluate_models(source='data', loss_bias=biases, want_probs=False)
    res_loss, res_acc, _ = g.evaluate_models(source='data', loss_bias=biases)
    assert none is None and same_bits(loss2, res_loss) and same_bits(acc2, res_acc)
    g.close()


def test_errors_leave_everything_untouched(stock_weights):
    lib = _lib.load()
    models = [stock_weights, synth.make_weights(13, (8,), seed=3), synth.make_weights(13, (32,), seed=4)]
    t = _lib.HipTrainer(models, 29, 13)
    x, y = dataset()
    K, n = 3, 4
    sentinel = np.float32(-77.0)
    loss, acc = np.full(K, sentinel), np.full(K, sentinel)
    probs = np.full(K * n, sentinel)
    grads = np.full(t.n_params_total, sentinel)
    theta = t.get_weights()
    idx = np.array([0, 1, 2, 3], dtype=np.int32)

    def hparams(rates=(0.2, 0.2, 0.2)):
        hp = (_lib.PeTrainHparams * K)()
        for m in range(K):
            hp[m] = _lib.PeTrainHparams(rates[m], 1, 0.7, LR, RHO, EPS, 0)
        return hp

    def step(idx_, n_, hp, loss_=loss):
        return lib.pe_trainer_step_models(t._h, ptr(idx_), n_, 0, hp, ptr(loss_))

    bias = np.full(K, 0.7, dtype=np.float32)

    def evaluate(source, x_=None, y_=None, n_=0, bias_=bias):
        return lib.pe_trainer_evaluate_models(t._h, source, ptr(x_), ptr(y_), n_, ptr(bias_), ptr(loss), ptr(acc), ptr(probs))

    invalid = [step(idx, n, hparams()),                                   # (no dataset yet)
               evaluate(_lib.TRAIN_SOURCE_DATA), evaluate(_lib.TRAIN_SOURCE_VALIDATION), evaluate(7, x[:n], y[:n], n)]
    t.set_data(x[:n], y[:n])
    invalid += [step(idx, n, None), step(idx, n, hparams(), None), step(None, n, hparams()), step(idx, 0, hparams()),
                step(np.array([0, 1, 4, 3], dtype=np.int32), n, hparams()), step(np.array([0, -1, 2, 3], dtype=np.int32), n, hparams()),
                evaluate(_lib.TRAIN_SOURCE_VALIDATION), evaluate(_lib.TRAIN_SOURCE_HOST, None, y[:n], n),
                evaluate(_lib.TRAIN_SOURCE_HOST, x[:n], None, n), evaluate(_lib.TRAIN_SOURCE_HOST, x[:n], y[:n], 0),
                evaluate(_lib.TRAIN_SOURCE_HOST, x[:n], np.array([0, 1, 1.5, 1], dtype=np.float32), n),
                evaluate(_lib.TRAIN_SOURCE_DATA, bias_=None),
                lib.pe_trainer_set_validation(t._h, ptr(x[:n]), ptr(np.array([0, 1, np.nan, 1], dtype=np.float32)), n),
                lib.pe_trainer_set_validation(t._h, None, ptr(y[:n]), n), lib.pe_trainer_set_validation(t._h, ptr(x[:n]), ptr(y[:n]), 0)]
    assert invalid == [_lib.PE_ERR_INVALID] * len(invalid)
    for bad in (1.0, float('nan')):                                       # in model 2 only: the message names it
        assert step(idx, n, hparams((0.2, 0.0, bad))) == _lib.PE_ERR_INVALID
        assert lib.pe_trainer_last_error(t._h).decode().startswith('model 2: dropout rate')
    # the one-network entry points on a trainer of several
    one_loss = np.full(1, sentinel)
    unsupported = [lib.pe_trainer_loss_grad(t._h, ptr(x[:n]), ptr(y[:n]), n, None, 0.7, ptr(one_loss), ptr(grads), ptr(probs)),
                   lib.pe_trainer_apply(t._h, ptr(np.ones(t.n_params_total, dtype=np.float32)), LR, RHO, EPS, 0),
                   lib.pe_trainer_step(t._h, ptr(idx), n, 0.2, 1, 0, 0.7, LR, RHO, EPS, 0, ptr(one_loss)),
                   lib.pe_trainer_evaluate(t._h, ptr(x[:n]), ptr(y[:n]), n, 0.7, ptr(one_loss), ptr(acc), ptr(probs))]
    assert unsupported == [_lib.PE_ERR_UNSUPPORTED] * len(unsupported)
    assert 'n_models = 3' in lib.pe_trainer_last_error(t._h).decode()
    for out in (loss, acc, probs, grads, one_loss):
        assert np.all(out == sentinel)
    assert same_bits(t.get_weights(), theta) and not t.get_accumulators().any()
    with pytest.raises(NotImplementedError, match='pe_trainer_loss_grad'):
        t.loss_grad(x[:n], y[:n])
    # and the trainer still works
    assert np.all(np.isfinite(t.step_models(idx, dropout_rate=(0.2, 0.0, 0.5)))) and t.get_accumulators().any()
    t.close()


FIT_CANDIDATES = ((8, 0.2, 0.7), (20, 0.0, 0.9), (32, 0.5, 0.5))


def fit_candidates():
    return [ModelParams(recurrent_units=u, dropout=d, loss_bias=b) for u, d, b in FIT_CANDIDATES]


@functools.lru_cache(maxsize=None)
def fit_task():
    return learning_task(200, 1) + learning_task(50, 2)


def single_fits(seeds, shuffle):
    from mycroft_precise_amd.train import Trainer, flatten_weights
    x, y, xv, yv = fit_task()
    out = []
    for params, seed in zip(fit_candidates(), seeds):
        tr = Trainer(params=params, seed=seed)
        hist = tr.fit(x, y, batch_size=64, epochs=2, validation_data=(xv, yv), shuffle=shuffle)
        out.append((hist, flatten_weights(tr.weights)))
        tr.close()
    return out


@pytest.mark.parametrize('seeds,shuffle', [(None, True), ((5, 6, 7), False)], ids=['group_seed_shuffled', 'own_seeds_in_order'])
def test_trainer_group_fit_is_trainer_fit(tmp_path, seeds, shuffle):
    from mycroft_precise_amd.network_runner import HipRunner
    from mycroft_precise_amd.train import TrainerGroup, flatten_weights
    x, y, xv, yv = fit_task()
    seed = 17
    want = single_fits([seed] * 3 if seeds is None else seeds, shuffle)
    seen = []
    group = TrainerGroup(fit_candidates(), seeds=seeds, seed=seed)
    assert len(group) == 3 and group.units == [8, 20, 32]
    hists = group.fit(x, y, batch_size=64, epochs=2, validation_data=(xv, yv), shuffle=shuffle,
                      callback=lambda epoch, logs: seen.append((epoch, [dict(l) for l in logs])))
    assert [e for e, _ in seen] == [0, 1] and all(len(logs) == 3 for _, logs in seen)
    weights = group.weights
    for m, (hist, flat) in enumerate(want):
        assert set(hists[m]) == set(hist) == {'loss', 'acc', 'val_loss', 'val_acc'}
        for key in hist:
            assert len(hists[m][key]) == 2 and hists[m][key] == hist[key], (m, key, hists[m][key], hist[key])
            assert [logs[m][key] for _, logs in seen] == hist[key]
        assert same_bits(flatten_weights(weights[m]), flat), m
    last = [h['val_loss'][-1] for h in hists]
    assert group.best() == group.best('val_loss') == int(np.argmin(last))
    assert group.best('val_acc') == int(np.argmax([h['val_acc'][-1] for h in hists]))
    # predict / evaluate: every candidate with its own loss_bias, equal to the last epoch's validation figures
    pred = group.predict(xv)
    assert pred.shape == (3, 50, 1)
    for m, (loss, acc) in enumerate(group.evaluate(xv, yv)):
        assert loss == hists[m]['val_loss'][-1] and acc == hists[m]['val_acc'][-1]
    if seeds is None:
        # save(m) -> HipRunner serves candidate m (test_trained_model_round_trip's comparison and bound)
        m = 2
        path = str(tmp_path / 'candidate.npz')
        group.save(m, path)
        loaded = load_weights(path)
        for a, b in zip(loaded['gru'][0] + (loaded['dense_kernel'], loaded['dense_bias']),
                        weights[m]['gru'][0] + (weights[m]['dense_kernel'], weights[m]['dense_bias'])):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        got = HipRunner(path).predict(x)
        assert float(np.abs(got - group.predict(x)[m]).max()) <= 1e-5
    group.close()
