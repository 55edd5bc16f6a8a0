"""GPU: sampled training -- pe_trainer_evaluate_indices, ``fit_resident(subset=...)``, the choice of
pe_trainer_sample_choose in both orders and ``SampledTrainer`` against the script's loop restated in sampled_reference.py.

Every comparison is equality.  The failing set is controlled exactly: predict, set ``y = (p > 0.5)``, then flip ``y`` at
chosen rows.  Rows are 3 x 4 floats and the network has 5 units wherever the row shape does not matter."""
import functools

import numpy as np
import pytest

import sampled_reference as ref
from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.model import ModelParams
from mycroft_precise_amd.train import SampledTrainer, Trainer

pytestmark = pytest.mark.gpu

T, F, H = 3, 4, 5
B = _lib.SAMPLE_BLOCK_ROWS                  # rows one selection block owns (PE_SAMPLE_BLOCK_ROWS)
SIZES = [1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 3, 64 * B + 5]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def weights(seed=1):
    return synth.make_weights(F, (H,), seed=seed)


def tiny_trainer(seed=1, w=None):
    return Trainer(w if w is not None else weights(), ModelParams(recurrent_units=H), seed=seed, n_features=T)


def rows(n, seed=0):
    return np.random.default_rng(seed).normal(0.0, 1.0, (n, T, F)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def predicted(n, seed=0, w_seed=1):
    """the probabilities of weights(w_seed) over rows(n, seed): computed once per shape, read-only"""
    t = _lib.HipTrainer(weights(w_seed), T, F)
    try:
        p = t.evaluate(rows(n, seed))[2]
    finally:
        t.close()
    p.setflags(write=False)
    return p


def targets_failing_at(p, failing):
    y = (p > 0.5).astype(np.float32)
    failing = np.asarray(sorted(failing), dtype=np.int64)
    y[failing] = 1.0 - y[failing]
    return y


def border_rows(n, max_new):
    """row 0, row n - 1, both sides of every wave (64) and block (B) border, and one dense run longer than max_new"""
    failing = {0, n - 1}
    for k in range(64, n, 64):
        failing.update((k - 1, k))
    run = min(n, max_new + 6)
    start = max(0, min(n - run, B - run // 2))          # across the first block border when the set reaches it
    failing.update(range(start, start + run))
    return failing


def walk(t, y, failing, order, eligible=None, calls=(0, 1, 50, 1024)):
    """calls of sample_choose on one state until nothing remains, each against numpy"""
    n = y.size
    eligible = np.ones(n, dtype=bool) if eligible is None else eligible
    fail = np.zeros(n, dtype=bool)
    fail[sorted(failing)] = True
    selected = []
    calls = list(calls)
    while True:
        max_new = calls.pop(0) if calls else 1024
        report, added, p = t.sample_choose(max_new, order, want_probs=True)
        assert np.array_equal((p > 0.5) != (y > 0.5), fail)
        mask = fail & eligible
        mask[selected] = False
        want = ref.lexsort_rows(np.flatnonzero(mask), p, y, order)[:max_new]
        assert added.dtype == np.int32 and added.tolist() == want.tolist()
        if order == 'index':
            assert np.all(np.diff(added) > 0)
        selected += want.tolist()
        assert report == {'n': n, 'n_correct': n - int(fail.sum()), 'n_failed': int((fail & eligible).sum()), 'n_remaining': int(mask.sum()),
                          'n_added': want.size, 'n_selected': len(selected)}
        assert t.sample_selected().tolist() == selected
        if max_new and report['n_remaining'] == report['n_added']:
            break
    report, added, _ = t.sample_choose(50, order)
    assert (report['n_remaining'], report['n_added'], added.size, report['n_selected']) == (0, 0, 0, len(selected))
    return selected


# ---- evaluate_indices ---------------------------------------------------------------------------------------------------
def some_indices(n, n_set, seed):
    idx = np.random.default_rng(seed).integers(0, n_set, n)
    idx[:min(n, n_set)] = np.arange(n_set)[::-1][:min(n, n_set)]        # descending
    if n > 1:
        idx[-1] = idx[0]                                                # repeated
    return idx


@pytest.mark.parametrize('validation', [False, True])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 33])
def test_evaluate_indices_equals_the_host_rows(n, validation):
    x, y = rows(40, 5), (np.random.default_rng(6).random(40) < 0.5).astype(np.float32)
    other_x, other_y = rows(7, 8), np.zeros(7, dtype=np.float32)
    t = _lib.HipTrainer(weights(), T, F)
    try:
        (t.set_validation if validation else t.set_data)(x, y)
        (t.set_data if validation else t.set_validation)(other_x, other_y)
        idx = some_indices(n, 40, n)
        loss, acc, probs = t.evaluate_indices(idx, loss_bias=0.7, validation=validation)
        want = t.evaluate_models(x[idx], y[idx], loss_bias=0.7)
    finally:
        t.close()
    assert np.array_equal(bits(loss), bits(want[0])) and np.array_equal(bits(acc), bits(want[1]))
    assert probs.shape == (1, n) and np.array_equal(bits(probs), bits(want[2]))


def test_evaluate_indices_of_two_networks():
    x, y = rows(40, 5), (np.random.default_rng(6).random(40) < 0.5).astype(np.float32)
    t = _lib.HipTrainer([weights(1), synth.make_weights(F, (H + 3,), seed=2)], T, F)
    try:
        t.set_data(x, y)
        idx = some_indices(33, 40, 2)
        got = t.evaluate_indices(idx, loss_bias=[0.7, 0.4])
        want = t.evaluate_models(x[idx], y[idx], loss_bias=[0.7, 0.4])
    finally:
        t.close()
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w))
    assert np.any(got[2][0] != got[2][1])


def test_evaluate_indices_refuses_an_index_outside_the_set_and_leaves_the_outputs():
    t = _lib.HipTrainer(weights(), T, F)
    try:
        t.set_data(rows(10), np.zeros(10, dtype=np.float32))
        for bad in (10, -1):
            idx = np.array([3, bad, 4], dtype=np.int32)
            bias = np.array([0.7], dtype=np.float32)
            loss, acc, probs = np.full(1, 7.0, np.float32), np.full(1, 7.0, np.float32), np.full(3, 7.0, np.float32)
            rc = t._lib.pe_trainer_evaluate_indices(t._h, _lib.TRAIN_SOURCE_DATA, idx.ctypes.data, 3, bias.ctypes.data, loss.ctypes.data,
                                                    acc.ctypes.data, probs.ctypes.data)
            assert rc == _lib.PE_ERR_INVALID
            assert 'indices[1] = %d' % bad in t._lib.pe_trainer_last_error(t._h).decode()
            assert loss[0] == acc[0] == 7.0 and np.all(probs == 7.0)
        with pytest.raises(ValueError, match='no resident validation set'):
            t.evaluate_indices([0], validation=True)
    finally:
        t.close()


# ---- fit_resident(subset) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shuffle', [False, True])
@pytest.mark.parametrize('size', [1, 17, 23])
def test_fit_resident_on_a_subset_equals_fit_on_its_rows(size, shuffle):
    x, y = rows(23, 3), (np.random.default_rng(4).random(23) < 0.5).astype(np.float32)
    if size == 23:
        ids = np.arange(23)
    else:
        ids = np.random.default_rng(size).permutation(23)[:size]
        ids[-1] = ids[0]                                                # a repeat (size 1: the row itself)
    a, b = tiny_trainer(seed=9), tiny_trainer(seed=9)
    try:
        a.set_data(x, y)
        ha = a.fit_resident(batch_size=5, epochs=2, shuffle=shuffle, subset=ids)
        hb = b.fit(x[ids], y[ids], batch_size=5, epochs=2, shuffle=shuffle)
        assert a.n_samples() == 23
        assert ha == hb and len(ha['loss']) == 2
        assert np.array_equal(bits(a._t.get_weights()), bits(b._t.get_weights()))
        assert np.array_equal(bits(a._t.get_accumulators()), bits(b._t.get_accumulators()))
        assert np.any(a._t.get_weights() != tiny_trainer(seed=9)._t.get_weights())
        with pytest.raises(ValueError):
            a.fit_resident(subset=[0, 23])
    finally:
        a.close()
        b.close()


# ---- choose -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', ['index', 'error'])
@pytest.mark.parametrize('n', SIZES)
def test_choose_against_numpy(n, order):
    """order index: ascending ids truncated at max_new in {0, 1, 50, 1024}, every call going on where the one before stopped.
    order error: the same walk against lexsort over the probabilities of the same call; duplicated rows give equal keys, and
    past one block (n > B) the choice takes at least two rounds"""
    x = rows(n).copy()
    failing = border_rows(n, 1024 if n > 1100 else 50)
    pairs = [(a, b) for a, b in ((63, 64), (B - 1, B), (B - 2, 2 * B)) if b < n - 1] + [(0, n - 1)] * (n > 1)
    for a, b in pairs:                                  # the later row a copy of the earlier one: both fail, with one key
        x[b] = x[a]
    t = _lib.HipTrainer(weights(), T, F)
    try:
        p = t.evaluate(x)[2]
        y = targets_failing_at(p, failing)
        t.set_data(x, y)
        for a, b in pairs:
            assert p[a] == p[b] and y[a] == y[b] and {a, b} <= failing
        selected = walk(t, y, failing, order)
    finally:
        t.close()
    assert sorted(selected) == sorted(failing)
    if order == 'error':
        for a, b in pairs:
            assert selected.index(a) + 1 == selected.index(b)          # equal keys: the lower row first


def test_choose_without_failing_rows_adds_nothing():
    n = 130
    t = _lib.HipTrainer(weights(), T, F)
    try:
        t.set_data(rows(n), targets_failing_at(predicted(n), []))
        for order in ('index', 'error'):
            report, added, _ = t.sample_choose(50, order)
            assert report == {'n': n, 'n_correct': n, 'n_failed': 0, 'n_remaining': 0, 'n_added': 0, 'n_selected': 0} and added.size == 0
        assert t.sample_selected().size == 0
    finally:
        t.close()


def test_choose_with_a_nan_network_counts_as_numpy_compares():
    n = 70
    w = weights()
    w['dense_bias'] = np.array([np.nan], dtype=np.float32)
    y = (np.random.default_rng(2).random(n) < 0.5).astype(np.float32)
    t = _lib.HipTrainer(w, T, F)
    try:
        t.set_data(rows(n), y)
        report, added, p = t.sample_choose(20, 'error', want_probs=True)
    finally:
        t.close()
    assert np.all(np.isnan(p))
    fail = (p > 0.5) != (y > 0.5)
    assert np.array_equal(fail, y > 0.5)                               # a NaN never exceeds 0.5
    assert report['n_correct'] == int((~fail).sum()) and report['n_failed'] == report['n_remaining'] == int(fail.sum()) > 20
    # every error is NaN, which ranks as +infinity: all keys tie, the lowest rows come first
    assert added.tolist() == ref.lexsort_rows(np.flatnonzero(fail), p, y, 'error')[:20].tolist() == np.flatnonzero(fail)[:20].tolist()


def test_choose_refusals_come_before_any_device_work():
    t = _lib.HipTrainer(weights(), T, F)
    try:
        with pytest.raises(ValueError, match='no resident training set'):
            t.sample_choose(5)
        with pytest.raises(ValueError, match='no resident training set'):
            t.sample_reset()
        t.set_data(rows(10), np.zeros(10, dtype=np.float32))
        with pytest.raises(NotImplementedError, match='max_new = 1025'):
            t.sample_choose(1025)
        with pytest.raises(ValueError, match='max_new = -1'):
            t.sample_choose(-1)
        with pytest.raises(ValueError, match='model = 1'):
            t.sample_choose(5, model=1)
        with pytest.raises(ValueError, match='order'):
            t.sample_choose(5, order='loss')
        report = _lib.PeSampleReport()
        assert t._lib.pe_trainer_sample_choose(t._h, 0, 5, 2, report, None, None) == _lib.PE_ERR_INVALID
        assert 'order = 2' in t._lib.pe_trainer_last_error(t._h).decode()
    finally:
        t.close()


# ---- eligible and reset -------------------------------------------------------------------------------------------------
def test_eligible_reset_set_data_and_append():
    n = 130
    x, p = rows(n), predicted(n)
    failing = [0, 5, 63, 64, 65, 100, 129]
    y = targets_failing_at(p, failing)
    eligible = np.ones(n, dtype=bool)
    eligible[[5, 64, 7]] = False                        # two failing rows and one that passes
    t = _lib.HipTrainer(weights(), T, F)
    try:
        t.set_data(x, y)
        t.sample_reset(eligible, [100, 0])
        assert t.sample_selected().tolist() == [100, 0]
        report, added, _ = t.sample_choose(0)
        assert report == {'n': n, 'n_correct': n - 7, 'n_failed': 5, 'n_remaining': 3, 'n_added': 0, 'n_selected': 2}
        for bad, why in (([63, 63], 'repeated'), ([63, 5], 'not an eligible row'), ([63, n], 'outside the set'), ([-1], 'outside the set')):
            with pytest.raises(ValueError, match=why):
                t.sample_reset(eligible, bad)
        with pytest.raises(ValueError):
            t.sample_reset(eligible[:-1])
        assert t.sample_selected().tolist() == [100, 0]                 # a refused reset leaves the state
        report, added, _ = t.sample_choose(2, 'index')
        assert added.tolist() == [63, 65] and report['n_remaining'] == 3 and report['n_selected'] == 4
        # appended rows are eligible and unselected; the rows before them keep their state
        more = rows(3, 77)
        more_y = 1.0 - (_lib.HipTrainer(weights(), T, F).evaluate(more)[2] > 0.5).astype(np.float32)
        t.append(more, more_y)
        report, added, _ = t.sample_choose(50, 'index')
        assert added.tolist() == [129, 130, 131, 132]
        assert report == {'n': n + 3, 'n_correct': n - 7, 'n_failed': 8, 'n_remaining': 4, 'n_added': 4, 'n_selected': 8}
        assert t.sample_selected().tolist() == [100, 0, 63, 65, 129, 130, 131, 132]
        # a new set: nothing selected, every row eligible
        t.set_data(x, y)
        assert t.sample_selected().size == 0
        report, added, _ = t.sample_choose(50, 'index')
        assert added.tolist() == failing and report['n_failed'] == report['n_remaining'] == 7
    finally:
        t.close()


@pytest.mark.parametrize('order', ['index', 'error'])
def test_model_argument_chooses_for_that_network(order):
    n = 200
    x = rows(n, 4)
    y = (np.random.default_rng(5).random(n) < 0.5).astype(np.float32)
    two, one = _lib.HipTrainer([weights(1), weights(2)], T, F), _lib.HipTrainer(weights(2), T, F)
    try:
        two.set_data(x, y)
        one.set_data(x, y)
        got, want = two.sample_choose(50, order, model=1, want_probs=True), one.sample_choose(50, order, want_probs=True)
        first = _lib.HipTrainer(weights(1), T, F).evaluate(x)[2]
    finally:
        two.close()
        one.close()
    assert got[0] == want[0] and got[0]['n_added'] == 50
    assert got[1].tolist() == want[1].tolist() and np.array_equal(bits(got[2]), bits(want[2]))
    assert np.any((first > 0.5) != (want[2] > 0.5))                     # the two networks disagree: model 0 would choose otherwise


# ---- end to end ---------------------------------------------------------------------------------------------------------
def run_both(make_trainer, x, y, order, tmp_path, cycles, epochs):
    a, b = make_trainer(), make_trainer()
    path, metrics_path = str(tmp_path / 'model.samples.json'), str(tmp_path / 'sampling-metrics.txt')
    try:
        st = SampledTrainer(a, x, y, num_sample_chunk=5, order=order)
        assert st.hashes == [ref.calc_sample_hash(i, o) for i, o in zip(x, y)]
        per_cycle = []
        results = st.run(cycles=cycles, epochs=epochs, batch_size=7, samples_file=path, metrics_file=metrics_path,
                         callback=lambda c, result: per_cycle.append(list(st.selected)))
        want_cycles, want_metrics, want_samples = ref.run(b, x, y, cycles, epochs, 7, 5, order)
        assert per_cycle == want_cycles and len(per_cycle[-1]) > 5
        assert st.metrics == want_metrics
        with open(metrics_path) as f:
            assert f.read().split('\n') == want_metrics
        assert set(train_file(path)) == want_samples == st.samples
        assert [r['added'] for r in results] == [want_cycles[0]] + [want_cycles[c][len(want_cycles[c - 1]):] for c in range(1, cycles)]
        assert all(len(r['history']['loss']) == epochs for r in results)
        assert np.array_equal(bits(a._t.get_weights()), bits(b._t.get_weights()))
        assert np.array_equal(bits(a._t.get_accumulators()), bits(b._t.get_accumulators()))
        # precise-train -sf FILE [-is] (train.py:146-157): the file's rows in file order, the others ascending
        chosen = [st.hash_to_ind[h] for h in train_file(path)]
        assert chosen == per_cycle[-1]
        others = sorted(set(st.hash_to_ind.values()) - set(chosen))
        for invert, picked in ((False, chosen), (True, others)):
            ha = st.fit_samples(path, invert=invert, batch_size=7, epochs=1)
            hb = b.fit(x[picked], y[picked], batch_size=7, epochs=1)
            assert ha == hb
            assert np.array_equal(bits(a._t.get_weights()), bits(b._t.get_weights()))
        assert st.selected == per_cycle[-1] and a.n_samples() == len(x)
    finally:
        a.close()
        b.close()


def train_file(path):
    from mycroft_precise_amd.train import read_samples_file
    return read_samples_file(path)


def duplicated(x, y, pairs):
    for a, b in pairs:
        assert a < b
        x[b], y[b] = x[a], y[a]
    return x, y


@pytest.mark.parametrize('order', ['index', 'error'])
def test_sampled_trainer_equals_the_scripts_loop(order, tmp_path):
    rng = np.random.default_rng(11)
    x = rng.normal(0.0, 1.0, (60, T, F))                               # float64, as TrainData.load hands them out
    y = (rng.random((60, 1)) < 0.5).astype(np.float64)
    x, y = duplicated(x, y, [(0, 59), (3, 4), (10, 40), (11, 41), (20, 21), (30, 58)])
    run_both(lambda: tiny_trainer(seed=7), x, y, order, tmp_path, cycles=4, epochs=2)


def test_sampled_trainer_at_the_stock_shape(stock_weights, tmp_path):
    rng = np.random.default_rng(12)
    x = rng.normal(0.0, 1.0, (40, 29, 13))
    y = (rng.random((40, 1)) < 0.5).astype(np.float64)
    x, y = duplicated(x, y, [(1, 39), (5, 6)])
    run_both(lambda: Trainer(stock_weights, ModelParams(recurrent_units=20), seed=7), x, y, 'error', tmp_path, cycles=2, epochs=1)


# ---- the script itself: tests/golden/train_sampled.npz (tools/make_script_fixtures.py) ----------------------------------------
def test_sampled_trainer_equals_the_scripts_own_cycles(stock_weights, tmp_path):
    """TrainSampledScript.choose_new_samples and write_sampling_metrics themselves, two cycles on the stock network: with
    num_sample_chunk below the remaining failures the choice is that many of the script's set, above it the whole set; the
    counts and the metrics lines are the script's."""
    from conftest import golden
    from test_gpu_parity import TOL_RAW
    from mycroft_precise_amd.train import flatten_weights, write_samples_file
    g = golden('train_sampled.npz')
    inputs, targets = g['inputs'], g['targets']
    n = len(inputs)
    assert np.abs(g['predictions'].astype(np.float64) - 0.5).min() > TOL_RAW

    def fresh(num_sample_chunk):
        trainer = Trainer(stock_weights, ModelParams(recurrent_units=20), seed=3)
        assert trainer._t.get_weights().tobytes() == flatten_weights(stock_weights).tobytes()
        st = SampledTrainer(trainer, inputs, targets, num_sample_chunk=num_sample_chunk, order='index')
        assert np.array_equal(np.array([st.hash_to_ind[h] for h in st.hashes]), g['hash_to_ind'])
        return st

    k0, remaining = int(g['num_sample_chunk_0']), g['remaining_0'].tolist()
    assert k0 < len(remaining)
    st = fresh(k0)
    report, _, probs = st.trainer._t.sample_choose(0, 'index', want_probs=True)                  # (max_new = 0: predictions alone)
    worst = float(np.abs(probs.astype(np.float64) - g['predictions'].reshape(-1).astype(np.float64)).max())
    print('%d rows, worst |p - the restated network\'s| %.3g' % (n, worst))
    assert worst <= TOL_RAW and report['n_added'] == 0
    result = st.cycle(epochs=1, batch_size=64)
    assert result['remaining'] == len(remaining) and len(result['added']) == k0 and set(result['added']) <= set(remaining)
    assert result['added'] == remaining[:k0]                                                    # order 'index'
    assert result['correct'] == float(g['correct_0']) and st.metrics == [str(g['line_0'])]
    st.trainer.close()

    # the second cycle from the script's own first choice (a samples file, as a continued run reads it)
    k1, remaining = int(g['num_sample_chunk_1']), g['remaining_1'].tolist()
    assert k1 > len(remaining)
    st = fresh(k1)
    path = str(tmp_path / 'model.samples.json')
    write_samples_file(path, [st.hashes[i] for i in g['chosen_0'].tolist()])
    st.load_samples(path)
    assert sorted(st.selected) == g['chosen_0'].tolist()
    result = st.cycle(epochs=1, batch_size=64)
    assert result['remaining'] == len(remaining) and sorted(result['added']) == remaining == g['chosen_1'].tolist()
    assert len(st.samples) == int(g['n_samples_1']) and result['correct'] == float(g['correct_1']) and st.metrics == [str(g['line_1'])]
    st.trainer.close()
