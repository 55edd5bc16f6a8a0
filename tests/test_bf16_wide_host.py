"""
CPU only: the stacked bf16 contract of tests/bf16_wide_reference.py and the rule test_bf16_wide.py judges the wide
bf16-operand kernel by.

  1. with one layer the stacked reference IS oracle.bf16_gru.predict: probabilities and operand digests, all four variants;
  2. the input conditions of every GPU case, as properties of the reference alone (the seeds in bf16_wide_reference.CASES
     are chosen so that they hold);
  3. S, the variants' largest distance on flip-free windows over every wide case, against the named constant S_WIDE;
  4. a mutation table: faults injected into the reference stay within the public 1e-2 of the float32 oracle and are rejected by
     the two-tier rule.
"""
import numpy as np
import pytest

import bf16_contract_common as cc
import bf16_wide_reference as wr
from mycroft_precise_amd import synth
from oracle import bf16_gru, keras_gru

TOL_PUBLIC = 1e-2


# ---- 1. one layer: bf16_gru.predict bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize('variant', wr.VARIANTS)
def test_one_layer_is_the_oracle(variant):
    w = synth.make_weights(n_in=wr.N_IN, units=(40,), seed=900)
    x = wr.normal_batch(16, 29, 8)
    p0, d0 = bf16_gru.predict(x, w, variant=variant, trace=True)
    p1, d1 = wr.predict(x, w, variant=variant, trace=True)
    assert np.array_equal(p0.view(np.uint64), p1.view(np.uint64))
    assert d0 == d1
    for kw in (dict(rounding='trunc'), dict(round_h=False), dict(bias_lo=False), dict(bump=(3, 7, 1.0))):
        kw1 = dict(kw, bump=(0,) + kw['bump']) if 'bump' in kw else kw
        assert np.array_equal(bf16_gru.predict(x, w, variant=variant, **kw), wr.predict(x, w, variant=variant, **kw1)), kw
    m0, _ = bf16_gru.flip_free(x, w)
    m1, _ = wr.flip_free(x, w)
    assert np.array_equal(m0, m1)


def test_layer_two_reads_the_rounded_state_of_layer_one():
    """B8 by construction: a two-layer network whose layer 2 is fed by hand with bf16(h1_t) sequences"""
    w = synth.make_weights(n_in=wr.N_IN, units=(40, 33), seed=900)
    x = wr.normal_batch(8, 6, 8)
    k, rk, b = (np.asarray(a, dtype=np.float32) for a in w['gru'][0])
    H = 40
    W, U = wr.round_bf16(k), wr.round_bf16(rk)
    hi, lo = wr.split_bias(b)
    xb = wr.round_bf16(x)
    h = np.zeros((8, H))
    seq = []
    for t in range(6):
        hb = wr.round_bf16(h)
        g = np.clip(0.2 * (xb[:, t] @ W[:, :2 * H] + (hi + lo)[:2 * H] + hb @ U[:, :2 * H]) + 0.5, 0, 1)
        z, r = g[:, :H], g[:, H:]
        c = xb[:, t] @ W[:, 2 * H:] + (hi + lo)[2 * H:] + wr.round_bf16(r * h) @ U[:, 2 * H:]
        h = z * h + (1 - z) * c
        seq.append(h.copy())
    seq = np.stack(seq, axis=1)                                  # float64 h1_t: rounding it gives values float32 holds exactly
    top = {'gru': [w['gru'][1]], 'dense_kernel': w['dense_kernel'], 'dense_bias': w['dense_bias']}
    want = bf16_gru.predict(wr.round_bf16(seq).astype(np.float32), top)
    assert np.array_equal(wr.predict(x, w), want)
    assert not np.array_equal(wr.predict(x, w, round_l2_in=False), want)


# ---- 2. + 3. input conditions and S -------------------------------------------------------------------------------------------
def wide_sets():
    """(label, network, windows, tier-1 case?) of every judged explicit batch of test_bf16_wide.py"""
    for units in wr.ONE_LAYER + wr.STACKED:
        yield 'case %s' % wr.case_id(units), wr.case_weights(units), wr.case_batch(units), True
    for units in [(64,), (40, 33)]:
        T = wr.CASES[units][0]
        yield 'ties %s tie batch' % wr.case_id(units), wr.tie_weights(units), wr.tie_batch(64, T), True
        yield 'ties %s normal batch' % wr.case_id(units), wr.tie_weights(units), wr.case_batch(units), True
    for units, (ns, bs) in wr.FULL_WINDOW.items():
        yield 'full %s' % wr.case_id(units), synth.make_weights(n_in=wr.N_IN, units=units, seed=ns), wr.normal_batch(17, 29, bs), False


_measured = {}


def measured():
    if not _measured:
        for label, w, x, tier1 in wide_sets():
            _measured[label] = (wr.Reference(x, w), w, x, tier1)
    return _measured


def test_input_conditions():
    """every tier-1 case has >= 32 flip-free windows among its 64; on every case the four variants lie within the case's
    one-ulp effect of each other over ALL windows (half of tier 2: a faithful evaluation has room); S against S_WIDE"""
    S = 0.0
    for label, (r, w, x, tier1) in measured().items():
        print('%-28s n=%2d T=%2d flip-free %2d  S=%.3g  variants apart over all windows %.3g  one-ulp effect %.3g' % (
            label, len(x), x.shape[1], r.n_free, r.spread, r.spread_all, r.effect))
        if tier1:
            assert len(x) == 64 and r.n_free >= wr.MIN_FLIP_FREE, label
        assert r.spread_all <= r.effect, label
        S = max(S, r.spread)
    print('S over all wide cases: %.3g (S_WIDE %.3g, TOL_TIGHT_WIDE %.3g)' % (S, wr.S_WIDE, wr.TOL_TIGHT_WIDE))
    assert S <= wr.S_WIDE
    assert wr.S_WIDE <= 2 * S                   # ... and the constant is the measurement, not a loose cap
    assert wr.TOL_TIGHT_WIDE == 8 * wr.S_WIDE


def test_full_windows_meet_the_public_bar_in_the_reference():
    for units, (ns, bs) in wr.FULL_WINDOW.items():
        r, w, x, _ = measured()['full %s' % wr.case_id(units)]
        far = float(np.abs(r.ref - keras_gru.predict(x, w)[:, 0]).max())
        print('full %s: the contract lies %.3g from the float32 oracle' % (wr.case_id(units), far))
        assert far <= TOL_PUBLIC


def test_every_faithful_variant_passes_the_rule():
    for label, (r, w, x, tier1) in measured().items():
        tol_flip = max(2 * r.effect, wr.TOL_TIGHT_WIDE)
        for v in wr.VARIANTS[1:]:
            assert wr.judge(r.outs[v], r.ref, r.mask if tier1 else np.zeros_like(r.mask), tol_flip)[0], (label, v)


def test_saturation_case_has_something_to_assert():
    for units, seed in wr.SATURATION_SEEDS.items():
        w = synth.make_weights(n_in=wr.N_IN, units=units, seed=seed, dense_scale=wr.SATURATION_DENSE_SCALE)
        p = np.stack([wr.predict(cc.huge_batch(), w, variant=v) for v in wr.VARIANTS]).astype(np.float32)
        same = np.all(p == p[0], axis=0) & ((p[0] == 0) | (p[0] == 1))
        print('huge features %s: %d of 16 windows saturated alike in every variant' % (wr.case_id(units), same.sum()))
        assert same.sum() >= 2


# ---- 4. the mutation table -------------------------------------------------------------------------------------------------------
FAULTS = {
    'layer-2 input left unrounded': dict(round_l2_in=False),
    'truncation instead of round to nearest even': dict(rounding='trunc'),
    'the bias lo half dropped': dict(bias_lo=False),
    'h and r*h left unrounded': dict(round_h=False),
}


@pytest.mark.parametrize('units', [(64,), (40, 33), (128, 100)], ids=wr.case_id)
def test_mutation_table(units):
    """each fault, applied to the reference itself, stays within 1e-2 of the float32 oracle -- the public bar lets it through --
    and is rejected by the two-tier rule against the unmutated reference"""
    w, x = wr.case_weights(units), wr.mutation_batch()
    r = wr.Reference(x, w)
    assert r.n_free >= wr.MIN_FLIP_FREE and r.spread <= wr.S_WIDE and r.spread_all <= r.effect
    f32 = keras_gru.predict(x, w)[:, 0]
    tol_flip = max(2 * r.effect, wr.TOL_TIGHT_WIDE)
    print('%s: the unmutated contract lies %.3g from the float32 oracle; TOL_TIGHT_WIDE %.3g, tier 2 %.3g' % (
        wr.case_id(units), np.abs(r.ref - f32).max(), wr.TOL_TIGHT_WIDE, tol_flip))
    for fault, kw in FAULTS.items():
        if 'round_l2_in' in kw and len(units) == 1:
            continue
        got = wr.predict(x, w, **kw)
        ok, outside, worst = wr.judge(got, r.ref, r.mask, tol_flip)
        old = float(np.abs(got - f32).max())
        print('%-8s %-46s from the float32 oracle %.3g | from the contract %.3g, %5.1f %% of flip-free windows outside TOL_TIGHT_WIDE: %s' % (
            wr.case_id(units), fault, old, worst, 100 * outside, 'passed' if ok else 'REJECTED'))
        assert old <= TOL_PUBLIC, (fault, old)
        assert not ok, fault
