"""
CPU: oracle/bf16_gru.py, the restated arithmetic contract of the bf16-operand network, and the rule by which
tests/test_bf16_contract.py holds the kernels to it.  Nothing here runs a kernel: the reference is tied to the float32 /
float64 oracle, its variants measure how far faithful evaluations of the contract lie apart (S, the flip-free share, the
one-ulp effect: the inputs of TOL_TIGHT and TOL_FLIP), and faults injected into the reference itself show that the
two-tier rule rejects what a plain <= 1e-2 comparison with the float32 oracle lets through.

    pytest tests/test_bf16_contract_host.py -s        prints every measured figure
"""
import functools

import numpy as np
import pytest

import bf16_contract_common as cc
import test_bf16_contract as gpu_tests
from oracle import bf16_gru, keras_gru

TOL_BF16 = 1e-2
TOL_TIGHT, S_MAX, TOL_FLIP_STOCK_STREAMS = gpu_tests.TOL_TIGHT, gpu_tests.S_MAX, gpu_tests.TOL_FLIP_STOCK_STREAMS


@functools.lru_cache(maxsize=None)
def stream_windows(n_in=13):
    x = cc.oracle_stream_windows(n_in)
    x.setflags(write=False)
    return x


def normal_set():
    return np.concatenate(cc.stock_normal_batches())


def stock_sets(stock):
    """the input sets of the GPU tests on the networks they meet them with: name -> (windows, weights)"""
    return {'a_streams': (stream_windows(), stock), 'b_normal': (normal_set(), stock), 'c_ties': (cc.tie_batch(), stock),
            'd_tie_weights_streams': (stream_windows(), cc.tie_weights()), 'd_tie_weights_normal': (normal_set(), cc.tie_weights()),
            'd_tie_weights_ties': (cc.tie_batch(), cc.tie_weights())}


SET_NAMES = ['a_streams', 'b_normal', 'c_ties', 'd_tie_weights_streams', 'd_tie_weights_normal', 'd_tie_weights_ties']


def test_round_bf16_is_round_to_nearest_even():
    """against the integer formula of the host packer (engine.hip: to_bf16), on random values, on ties of both parities,
    at the overflow to inf and on non-finite values"""
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.normal(0, 3, 4000).astype(np.float32), cc.tie_batch().reshape(-1)[:4000],
                        np.array([0.0, -0.0, 3.4e38, -3.4e38, 3.38e38, 1e-30, np.inf, -np.inf], dtype=np.float32)])
    u = v.view(np.uint32).astype(np.uint64)
    want = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)
    got = bf16_gru.round_bf16(v)
    assert np.array_equal(bf16_gru.bf16_bits(got), want)
    assert np.isinf(got[-6]) and np.isinf(got[-5]) and np.isfinite(got[-4])          # 3.4e38 -> inf, 3.38e38 stays
    assert np.isnan(bf16_gru.round_bf16(np.float32(np.nan)))
    # a float64 value is rounded ONCE (not via float32): 1 + 2^-8 + 2^-40 lies above the tie, float32 would put it ON the tie
    assert bf16_gru.round_bf16(1.0 + 2.0 ** -8 + 2.0 ** -40) == 1.0 + 2.0 ** -7
    assert bf16_gru.round_bf16(1.0 + 2.0 ** -8) == 1.0 and bf16_gru.round_bf16(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6
    t = bf16_gru.round_bf16(v[:8000], 'trunc')
    assert np.array_equal(bf16_gru.bf16_bits(t), (v[:8000].view(np.uint32) >> 16).astype(np.uint16))
    # the three rounding modes give three different operands on the tie batch
    ties = cc.tie_batch().reshape(-1)
    up = ties.view(np.uint32) >> 16
    rne = bf16_gru.bf16_bits(bf16_gru.round_bf16(ties))
    assert np.array_equal(rne != up, (up & 1) == 1) and 0.45 < np.mean(rne != up) < 0.55


@pytest.mark.parametrize('delta', [False, True])
def test_with_the_identity_for_rounding_it_is_the_float64_oracle(stock_weights, delta):
    """the same operation: rounding='none' against keras_gru.predict(dtype=float64), to 1e-12"""
    for x, w in ((stream_windows()[::7], stock_weights), (normal_set(), stock_weights), (cc.normal_batch(17, 5), cc.case_weights(7, 5, False))):
        if delta:
            w = cc.case_weights(20, x.shape[2], True) if x.shape[2] == 13 else cc.case_weights(7, 5, True)
            want = keras_gru.predict(cc.with_deltas(x), w, dtype=np.float64)[:, 0]
        else:
            want = keras_gru.predict(x, w, dtype=np.float64)[:, 0]
        got = bf16_gru.predict(x, w, use_delta=delta, rounding='none')
        assert np.abs(got - want).max() <= 1e-12
        if delta:       # an explicit batch that carries its delta columns is the same network
            assert np.abs(bf16_gru.predict(cc.with_deltas(x), w, rounding='none') - want).max() <= 1e-12


def test_delta_from_float32_rows_and_from_bf16_rows_differ():
    """B4 / B5: the reference models both, and they are different operands"""
    w = cc.case_weights(20, 13, True)
    x = stream_windows()[-43:]
    a = bf16_gru.predict(x, w, use_delta=True, rows='f32')
    b = bf16_gru.predict(x, w, use_delta=True, rows='bf16')
    assert np.abs(a - b).max() > 100 * TOL_TIGHT
    # bf16 rows: what the ring holds is already rounded, and rounding twice changes nothing
    xr = bf16_gru.round_bf16(x).astype(np.float32)
    assert np.array_equal(bf16_gru.predict(xr, w, use_delta=True, rows='bf16'), b)
    # float32 rows of an explicit batch: only rounded
    assert np.array_equal(bf16_gru.predict(cc.with_deltas(x), w), a)


@pytest.mark.parametrize('name', [n for n in SET_NAMES if n != 'd_tie_weights_normal'])      # ((d) is its weights; set (b) is judged on the stock network)
def test_contract_within_1e2_of_the_float32_oracle(stock_weights, name):
    """With rounding the reference stays within the product's public bf16 tolerance of the float32 oracle: a_streams 5.4e-3,
    b_normal 9.9e-3, c_ties 3.3e-3, tie weights on the streams 4.4e-3 and on the tie batch 3.1e-3.  For set (b) that holds by
    the choice of its seeds only (bf16_contract_common.STOCK_B_SEEDS); the next test says what unselected seeds give."""
    x, w = stock_sets(stock_weights)[name]
    d = float(np.abs(bf16_gru.predict(x, w) - keras_gru.predict(x, w)[:, 0]).max())
    print('%-24s contract vs float32 oracle: %.3g' % (name, d))
    assert d <= TOL_BF16


def test_shifted_normal_features_are_why_the_seeds_of_set_b_are_chosen(stock_weights):
    """A finding about the arithmetic, not about a kernel, written down so that the chosen seeds hide nothing: on normal(0, 2)
    features with x[..., 0] -= 20 the bf16 CONTRACT ITSELF leaves the 1e-2 bar of the float32 oracle on about one window in
    seven (10 unselected seeds x 68 windows: the share and the largest distance are printed), while the same batches without
    the shift stay within it (<= 5.1e-3).  The bar is a statement about MFCC-like rows."""
    d, plain = [], []
    for seed in range(100, 110):
        x = np.concatenate([cc.normal_batch(n, seed=seed) for n in (1, 17, 50)])
        d.append(np.abs(bf16_gru.predict(x, stock_weights) - keras_gru.predict(x, stock_weights)[:, 0]))
        x = x.copy()
        x[..., 0] += np.float32(20)
        plain.append(np.abs(bf16_gru.predict(x, stock_weights) - keras_gru.predict(x, stock_weights)[:, 0]))
    d, plain = np.concatenate(d), np.concatenate(plain)
    print('shifted: %.1f %% of %d windows beyond 1e-2, largest %.3g; unshifted: largest %.3g' % (100 * (d > TOL_BF16).mean(), d.size, d.max(), plain.max()))
    assert (d > TOL_BF16).mean() > 0.05 and plain.max() <= TOL_BF16


def test_input_conditions_of_the_stock_sets(stock_weights):
    """>= 95 % of the windows of every input set are flip-free, on those the variants agree to within S <= S_MAX (what
    TOL_TIGHT = 8 S_MAX is made of); the one-ulp effect of every set is printed, and for the stock network on the
    streamed rows it is what TOL_FLIP_STOCK_STREAMS is made of."""
    for name, (x, w) in stock_sets(stock_weights).items():
        r = cc.Reference(x, w)
        eff = bf16_gru.one_ulp_effect(x, w, n_pairs=8 if name == 'a_streams' else 5)
        print('%-24s n=%4d flip-free %.4f  S=%.3g  spread over all windows %.3g  one-ulp effect %.3g%s' % (
            name, len(x), r.share, r.spread, bf16_gru.spread(r.outs, np.ones_like(r.mask)), eff,
            '   (2 x effect >= 1e-2: tier 2 adds nothing over TOL_BF16 here)' if 2 * eff >= TOL_BF16 else ''))
        assert r.share >= cc.MIN_FLIP_FREE, name
        assert r.spread <= S_MAX, name
        if name == 'a_streams':
            assert 2 * eff <= TOL_FLIP_STOCK_STREAMS < TOL_BF16
            rb = cc.Reference(x, w, rows='bf16')
            assert rb.share >= cc.MIN_FLIP_FREE and rb.spread <= S_MAX


def case_sets(units, n_in, delta):
    xb, xc = cc.case_batches(units, n_in, delta)
    sets = [('a rows=f32', stream_windows(n_in), dict(use_delta=delta, rows='f32'))]
    if delta:
        sets.append(('a rows=bf16', stream_windows(n_in), dict(use_delta=True, rows='bf16')))
    return sets + [('b', np.concatenate(xb), {}), ('c', xc, {})]


CASES = [(u, f, d) for _, u, f in gpu_tests.NETS[:7] for d in (False, True) if not (d and f > 14)]


@pytest.mark.parametrize('units,n_in,delta', CASES)
def test_input_conditions_of_the_cases(units, n_in, delta):
    """the same two conditions for the network and the input sets of every GPU case"""
    w = cc.case_weights(units, n_in, delta)
    for name, x, kw in case_sets(units, n_in, delta):
        r = cc.Reference(x, w, **kw)
        print('%2d x %2d delta=%d %-12s n=%4d flip-free %.4f  S=%.3g' % (units, n_in, delta, name, len(x), r.share, r.spread))
        assert r.share >= cc.MIN_FLIP_FREE, name
        assert r.spread <= S_MAX, name


def test_input_conditions_of_the_three_models():
    from mycroft_precise_amd import synth
    for s in cc.MODEL_SEEDS:
        w = synth.make_weights(seed=s)
        for name, x in (('a', stream_windows()), ('b 50', cc.stock_normal_batches()[2])):
            for rows in ('f32', 'bf16'):
                r = cc.Reference(x, w, rows=rows)
                print('model seed %d %-5s rows=%s flip-free %.4f  S=%.3g' % (s, name, rows, r.share, r.spread))
                assert r.share >= cc.MIN_FLIP_FREE and r.spread <= S_MAX


def test_input_conditions_of_the_row_sequences_and_the_general_front_end():
    """the recording of the evaluate case, the six clips of the score_clips case and the streams behind the general front
    end, on the oracle's MFCC rows"""
    from oracle import listener as ol
    sets = [('evaluate', cc.evaluate_windows(ol.vectorize_raw(cc.evaluate_audio(), ol.Params()))),
            ('score_clips', np.stack([ol.vectorize(c, ol.Params()) for c in cc.clips()]).astype(np.float32))]
    assert sets[0][1].shape == (25, 29, 13) and sets[1][1].shape == (6, 29, 13)
    for delta in (False, True):
        w = cc.case_weights(20, 13, delta)
        for name, x in sets:
            r = cc.Reference(x, w, use_delta=delta)
            print('%-12s delta=%d n=%3d flip-free %.4f  S=%.3g' % (name, delta, len(x), r.share, r.spread))
            assert r.share >= cc.MIN_FLIP_FREE and r.spread <= S_MAX, (name, delta)
    x = cc.oracle_stream_windows(13, **cc.GENERAL_FRONT_END)
    for rows in ('f32', 'bf16'):
        r = cc.Reference(x, cc.case_weights(20, 13, False), rows=rows)
        print('general front end rows=%s n=%3d flip-free %.4f  S=%.3g' % (rows, len(x), r.share, r.spread))
        assert r.share >= cc.MIN_FLIP_FREE and r.spread <= S_MAX, rows


def test_edge_inputs_saturate_in_the_reference(stock_weights):
    """the saturation case of the GPU test has something to assert: windows that every variant puts at exactly 0.0 / 1.0"""
    want = cc.saturated(cc.huge_batch(), stock_weights)
    print('huge features: %d of 16 windows at 0.0, %d at 1.0, %d not saturated alike' % ((want == 0).sum(), (want == 1).sum(), np.isnan(want).sum()))
    assert (want == 0).sum() >= 2 and (want == 1).sum() >= 2


# ---- the mutation table ----------------------------------------------------------------------------------------------
def _mutated_weights(w, what):
    k, rk, b = (a.copy() for a in w['gru'][0])
    if what == 'bias_entry':
        b[59] = 0
    elif what == 'weight':
        k[3, 7] = 0
    elif what == 'rec_weight':
        rk[5, 41] = 0
    elif what == 'rows':
        k[[2, 3]] = k[[3, 2]]
    out = dict(w)
    out['gru'] = [(k, rk, b)]
    return out


def _drop_feature(x):
    x = x.copy()
    x[..., 4] = 0
    return x


# fault -> (mutated evaluation of the reference, does a plain <= 1e-2 comparison with the float32 oracle catch it on the
# 70-window batch of test_bf16_network_within_1e2_of_oracle; None: not asserted, only printed)
FAULTS = {
    'one bias entry dropped (bias[59] = 0)': (lambda x, w: bf16_gru.predict(x, _mutated_weights(w, 'bias_entry')), False),
    'the bias lo half dropped': (lambda x, w: bf16_gru.predict(x, w, bias_lo=False), False),
    'operands truncated instead of rounded to nearest even': (lambda x, w: bf16_gru.predict(x, w, rounding='trunc'), None),
    'h operand left unrounded': (lambda x, w: bf16_gru.predict(x, w, round_h=False), None),
    'one zeroed kernel weight': (lambda x, w: bf16_gru.predict(x, _mutated_weights(w, 'weight')), None),
    'one zeroed recurrent weight': (lambda x, w: bf16_gru.predict(x, _mutated_weights(w, 'rec_weight')), None),
    'a dropped feature': (lambda x, w: bf16_gru.predict(_drop_feature(x), w), True),
    'swapped kernel rows': (lambda x, w: bf16_gru.predict(x, _mutated_weights(w, 'rows')), True),
}


def test_mutation_table(stock_weights):
    """Every fault, applied to the reference itself, is rejected by the two-tier rule against the unmutated reference -- on
    the streamed rows (a), on the normal batches (b) and on the 70-window batch the 1e-2 test of the product uses --, and
    tier 1 alone rejects each.  The printout shows what a plain <= 1e-2 comparison with the float32 oracle makes of the same
    faults: on the 70-window batch it PASSES a dropped bias entry and a dropped bias lo half (asserted)."""
    sets = dict(stock_sets(stock_weights))
    sets = {'a_streams': sets['a_streams'], 'b_normal': sets['b_normal'],
            'batch70': (np.random.default_rng(8).normal(0, 2, (70, 29, 13)).astype(np.float32), stock_weights)}
    for set_name, (x, w) in sets.items():
        r = cc.Reference(x, w)
        tol_flip = TOL_FLIP_STOCK_STREAMS if set_name == 'a_streams' else 2 * bf16_gru.one_ulp_effect(x, w, n_pairs=5)
        f32 = keras_gru.predict(x, w)[:, 0]
        print('%-10s n=%d flip-free %.3f, the unmutated contract lies %.3g from the float32 oracle; TOL_TIGHT %.3g TOL_FLIP %.3g' % (
            set_name, len(x), r.share, np.abs(r.ref - f32).max(), TOL_TIGHT, tol_flip))
        for v in bf16_gru.VARIANTS[1:]:
            assert cc.judge(r.outs[v], r.ref, r.mask, TOL_TIGHT, tol_flip)[0], v          # every faithful evaluation passes
        for fault, (run, old_bar_catches) in FAULTS.items():
            got = run(x, w)
            ok, outside, worst = cc.judge(got, r.ref, r.mask, TOL_TIGHT, tol_flip)
            old = float(np.abs(got - f32).max())
            print('%-10s %-54s from the float32 oracle %.3g (%s by <= 1e-2) | from the contract %.3g, %5.1f %% of flip-free windows outside TOL_TIGHT: %s' % (
                set_name, fault, old, 'PASSED' if old <= TOL_BF16 else 'caught', worst, 100 * outside, 'passed' if ok else 'REJECTED'))
            assert not ok, (set_name, fault)
            assert outside > cc.MAX_OUTSIDE, (set_name, fault)            # tier 1 alone sees each of them
            if set_name == 'batch70' and old_bar_catches is not None:
                assert (old > TOL_BF16) == old_bar_catches, (fault, old)
