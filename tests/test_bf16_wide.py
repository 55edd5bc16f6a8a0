"""
-m gpu: the wide / stacked bf16-operand network (gru_precision='bf16' at 33-256 units, one or two layers;
csrc/gru_wide_bf16_device.h) against the bf16-exact stacked reference of tests/bf16_wide_reference.py.

The rule (bf16_wide_reference.judge).  ``ref`` is the reference's 'f64' variant on the windows the device saw, ``mask`` the
windows on which its four variants round every operand of every layer alike ("flip-free").
  tier 1   |got - ref| <= TOL_TIGHT_WIDE on all but at most 3 % of the flip-free windows
  tier 2   |got - ref| <= max(2 x one-ulp effect of the case, TOL_TIGHT_WIDE) on every window
Flip-free windows fall with width x window length, so tier 1 is judged on SHORT windows (8 / 6 / 4 timesteps, where every
case keeps >= 32 flip-free windows of 64: test_bf16_wide_host.py); full 29-step windows -- explicit batches, streaming, the
offline evaluator -- are judged by tier 2 and by the public bar, <= 1e-2 from the float32 oracle.  Every tolerance comes from
the reference alone; every check prints its figures before it asserts.
"""
import faulthandler
import warnings

import numpy as np
import pytest

import bf16_contract_common as cc
import bf16_wide_reference as wr
from mycroft_precise_amd import params as P
from mycroft_precise_amd import synth
from oracle import keras_gru

pytestmark = pytest.mark.gpu

TOL_PUBLIC = 1e-2
TIME_LIMIT_S = 120              # per test: a hung launch ends the whole run instead of the next test starting on the card


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def params_for(T, **kw):
    hpr = P.pr.copy()
    hpr.__dict__.update(buffer_t=wr.BUFFER_T[T], **kw)
    assert hpr.n_features == T
    return hpr


def engine(weights, T=29, n_streams=1, gru='bf16', ring='f32', **kw):
    from mycroft_precise_amd._lib import HipEngine
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return HipEngine(params_for(T, **kw), weights, n_streams=n_streams, gru_precision=gru, ring_precision=ring)


_refs = {}


def reference(x, weights):
    """computed once per (windows, network)"""
    key = (x.tobytes(), weights['gru'][0][0].tobytes(), weights['gru'][-1][2].tobytes())
    if key not in _refs:
        if len(_refs) > 12:
            _refs.clear()
        _refs[key] = wr.Reference(x, weights)
    return _refs[key]


def check(label, got, x, weights, idx=None, tier1=True, public=False):
    """the two-tier rule on one set of windows (``idx``: the windows of x that ``got`` holds, in order)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    r = reference(x, weights)
    idx = np.arange(len(x)) if idx is None else np.asarray(idx)
    ref, mask = r.ref[idx], r.mask[idx]
    tol_flip = max(2 * r.effect, wr.TOL_TIGHT_WIDE)
    ok, outside, worst = wr.judge(got, ref, mask if tier1 else np.zeros_like(mask), tol_flip)
    d = np.abs(np.asarray(got, dtype=np.float64).reshape(-1) - ref)
    print('%-40s n=%3d flip-free %3d  outside TOL_TIGHT_WIDE (%.3g) %.4f  worst flip-free %.3g  worst %.3g  (tier 2: %.3g)%s' % (
        label, len(ref), mask.sum(), wr.TOL_TIGHT_WIDE, float((~(d[mask] <= wr.TOL_TIGHT_WIDE)).mean()) if mask.any() else 0.0,
        float(d[mask].max()) if mask.any() else 0.0, worst, tol_flip, '' if tier1 else '  [tier 2 only]'))
    if public:
        far = float(np.abs(np.asarray(got, dtype=np.float64).reshape(-1) - keras_gru.predict(x, weights)[idx, 0]).max())
        print('%-40s from the float32 oracle %.3g (reference: %.3g)' % (label, far, float(np.abs(r.ref - keras_gru.predict(x, weights)[:, 0]).max())))
        assert far <= TOL_PUBLIC, (label, far)
    assert ok, (label, 'flip-free outside TOL_TIGHT_WIDE: %.4f (cap %.2f); worst %.3g (tier 2 %.3g)' % (outside, wr.MAX_OUTSIDE, worst, tol_flip))
    return r


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the engine exists -------------------------------------------------------------------------------------------------
def test_wide_bf16_engine_is_created():
    eng = engine(synth.make_weights(units=(64,), seed=900))
    info = eng.info()
    assert info.gru_precision == 1 and info.units == 64
    assert eng.gru_tiling() == 0
    eng.set_gru_tiling(0)
    eng.close()


# ---- tier 1 and tier 2 on short windows: pe_predict (kFeats), one lane, a ragged tile, four tiles --------------------------
@pytest.mark.parametrize('units', wr.ONE_LAYER + wr.STACKED, ids=wr.case_id)
def test_predict_by_width(units):
    w, x = wr.case_weights(units), wr.case_batch(units)
    eng = engine(w, x.shape[1])
    got = np.concatenate([eng.predict(x[:n])[:, 0] for n in (1, 17, 64)])
    eng.close()
    check('predict %s 1 + 17 + 64' % wr.case_id(units), got, x, w, idx=np.concatenate([np.arange(n) for n in (1, 17, 64)]))


# ---- ties: RNE against half-up and truncation, features and both layers' weights -------------------------------------------
@pytest.mark.parametrize('units', [(64,), (40, 33)], ids=wr.case_id)
def test_ties_in_features_and_weights(units):
    T = wr.CASES[units][0]
    w = wr.tie_weights(units)
    eng = engine(w, T)
    xt, xn = wr.tie_batch(64, T), wr.case_batch(units)
    got_t, got_n = eng.predict(xt)[:, 0], eng.predict(xn)[:, 0]
    eng.close()
    check('tie weights, tie batch %s' % wr.case_id(units), got_t, xt, w)
    check('tie weights, normal batch %s' % wr.case_id(units), got_n, xn, w)


# ---- 29 timesteps: tier 2 and the public bar ----------------------------------------------------------------------------------
@pytest.mark.parametrize('units', list(wr.FULL_WINDOW), ids=wr.case_id)
def test_full_windows(units):
    ns, bs = wr.FULL_WINDOW[units]
    w = synth.make_weights(n_in=wr.N_IN, units=units, seed=ns)
    x = wr.normal_batch(17, 29, bs)
    eng = engine(w)
    got = eng.predict(x)[:, 0]
    eng.close()
    check('29 timesteps %s' % wr.case_id(units), got, x, w, tier1=False, public=True)


# ---- edges: the expected values are the reference's ------------------------------------------------------------------------
def saturated(x, weights):
    p = np.stack([wr.predict(x, weights, variant=v) for v in wr.VARIANTS]).astype(np.float32)
    same = np.all(p == p[0], axis=0) & ((p[0] == 0) | (p[0] == 1))
    return np.where(same, p[0], np.float32(np.nan)).astype(np.float32)


@pytest.mark.parametrize('units', [(64,), (40, 33)], ids=wr.case_id)
def test_saturation_and_non_finite_features(units):
    w = synth.make_weights(n_in=wr.N_IN, units=units, seed=wr.SATURATION_SEEDS[units], dense_scale=wr.SATURATION_DENSE_SCALE)
    eng = engine(w)
    x = cc.huge_batch()
    want = saturated(x, w)
    sat = ~np.isnan(want)
    assert sat.sum() >= 2, want
    got = eng.predict(x)[:, 0]
    print('saturated windows: %d of %d; want' % (sat.sum(), len(x)), want[sat], 'got', got[sat])
    assert np.array_equal(got[sat], want[sat])
    clean, dirty, hit = cc.non_finite_batch()
    a, b = eng.predict(clean)[:, 0], eng.predict(dirty)[:, 0]
    eng.close()
    others = np.ones(len(clean), dtype=bool)
    others[hit] = False
    assert np.array_equal(bits(a[others]), bits(b[others]))                  # no lane leaks into its neighbours
    assert np.all(~np.isfinite(b[hit]) | (b[hit] == 0) | (b[hit] == 1)), b[hit]


# ---- streaming (kRing) through BatchedListener; a masked clear; the offline evaluator (kRows) ------------------------------
N_STREAMS, N_UPDATES, CHUNK = 21, 36, 1024


def stream_pcm():
    return synth.batch_pcm(N_STREAMS, N_UPDATES, CHUNK)


@pytest.mark.parametrize('units', [(128, 100), (256, 256)], ids=wr.case_id)
def test_streaming_through_batched_listener(units):
    from mycroft_precise_amd.network_runner import BatchedListener
    w = synth.make_weights(n_in=wr.N_IN, units=units, seed=900)
    pcm = stream_pcm()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        lis = [BatchedListener(w, N_STREAMS, gru_precision='bf16') for _ in range(2)]
    mask = (np.arange(N_STREAMS) % 3 == 1)
    fresh = None
    for u in range(N_UPDATES):
        out = [li.update_raw(pcm[u]) for li in lis]
        if fresh is None:
            assert np.array_equal(bits(out[0]), bits(out[1]))
        else:                                                # after the masked clear: those streams started over, the others did not notice
            started = fresh.update_raw(pcm[u])
            assert np.array_equal(bits(out[1][~mask]), bits(out[0][~mask])) and np.array_equal(bits(out[1][mask]), bits(started[mask]))
        if u in (23, N_UPDATES - 1):
            check('streaming %s after update %d' % (wr.case_id(units), u + 1), out[0], lis[0].engine.get_vectors(), w, tier1=False, public=True)
        if u == 23:
            lis[1].clear(mask)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                fresh = BatchedListener(w, N_STREAMS, gru_precision='bf16')
    for li in lis + [fresh]:
        li.engine.close()


def test_offline_evaluator_on_one_recording():
    w = synth.make_weights(n_in=wr.N_IN, units=(128, 100), seed=900)
    eng = engine(w)
    audio = cc.evaluate_audio()                                                    # 4 s
    x = cc.evaluate_windows(eng.vectorize_raw(audio))                              # the float32 rows the network read
    got = eng.evaluate(audio, 2)
    eng.close()
    assert got.shape == (len(x), 1)
    check('evaluate(4 s, hop 2) 128x100', got[:, 0], x, w, tier1=False, public=True)


# ---- bit-level properties of the new path -------------------------------------------------------------------------------------
def test_same_call_twice_and_any_batch_any_position():
    """a window's bits depend neither on the batch nor on its position, ragged last tile included"""
    units = (100,)
    w, x = wr.case_weights(units), wr.case_batch(units)[:37]                       # three tiles, the last with 5 windows
    eng = engine(w, x.shape[1])
    a, b = eng.predict(x), eng.predict(x)
    assert np.array_equal(bits(a), bits(b))
    for i in range(len(x)):
        assert bits(eng.predict(x[i:i + 1]))[0, 0] == bits(a)[i, 0], i
    assert np.array_equal(bits(eng.predict(x[5:30])), bits(a)[5:30])
    eng.close()
    w2, x2 = wr.case_weights((256, 256)), wr.case_batch((256, 256))[:21]
    eng = engine(w2, x2.shape[1])
    a = eng.predict(x2)
    assert np.array_equal(bits(eng.predict(x2)), bits(a))
    assert np.array_equal(bits(np.concatenate([eng.predict(x2[i:i + 1]) for i in (0, 15, 16, 20)])), bits(a)[[0, 15, 16, 20]])
    eng.close()


@pytest.mark.parametrize('units', [(64,), (72, 200)], ids=wr.case_id)
def test_update_many_and_subset_updates(units):
    w = synth.make_weights(n_in=wr.N_IN, units=units, seed=900)
    pcm = stream_pcm()[:12]
    n = N_STREAMS
    plain, many, subset = (engine(w, n_streams=n) for _ in range(3))
    many.reserve_updates(4, CHUNK)
    ids = np.arange(n, dtype=np.int32)
    for u in range(0, 12, 4):
        a = np.stack([plain.update(pcm[v]) for v in range(u, u + 4)])
        assert np.array_equal(bits(many.update_many(pcm[u:u + 4])), bits(a))        # update_many == consecutive updates
        s = np.stack([subset.update_subset(ids, pcm[v]) for v in range(u, u + 4)])
        assert np.array_equal(bits(s), bits(a))                                     # a subset of all streams == the full update
    assert a.min() > 0 and a.max() < 1 and np.unique(bits(a[-1])).size > n // 2
    for e in (plain, many, subset):
        e.close()
    # a random half at random cadences against one engine per stream
    n = 6
    rng = np.random.default_rng(5)
    together = engine(w, n_streams=n)
    alone = [engine(w, n_streams=1) for _ in range(n)]
    fed = np.zeros(n, dtype=int)
    streams = [synth.stream_pcm(s, 40 * CHUNK).reshape(40, CHUNK) for s in range(n)]
    for _ in range(40):
        pick = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int32)
        chunk = np.stack([streams[s][fed[s]] for s in pick])
        got = together.update_subset(pick, chunk)
        want = np.array([alone[s].update(streams[s][fed[s]].reshape(1, -1))[0] for s in pick], dtype=np.float32)
        assert np.array_equal(bits(got), bits(want))
        fed[pick] += 1
    together.close()
    for e in alone:
        e.close()


def test_two_models_equal_two_engines_and_set_weights_equals_fresh():
    units = (128, 100)
    w0, w1 = (synth.make_weights(n_in=wr.N_IN, units=units, seed=s) for s in (900, 901))
    pcm = stream_pcm()[:32]
    x = wr.normal_batch(17, 29, 8)
    both = engine([w0, w1], n_streams=N_STREAMS)
    one = [engine(wm, n_streams=N_STREAMS) for wm in (w0, w1)]
    for u in range(32):
        out = both.update(pcm[u])
        assert out.shape == (2, N_STREAMS)
        for m in range(2):
            assert np.array_equal(bits(out[m]), bits(one[m].update(pcm[u])))
    p = both.predict(x)
    for m in range(2):
        assert np.array_equal(bits(p[m]), bits(one[m].predict(x)))
    both.close()
    # set_weights on a live engine == an engine created with those weights (streams' state stays)
    one[0].set_weights(w1)
    assert np.array_equal(bits(one[0].predict(x)), bits(one[1].predict(x)))
    assert np.array_equal(bits(one[0].update(pcm[0])), bits(one[1].update(pcm[0])))
    for e in one:
        e.close()


def test_padding_is_inert():
    """100 units (run at 128 with the packer's zero padding) == the same network written out at 128 units with zero weights"""
    w = wr.case_weights((100,))
    H, Hp = 100, 128
    k, rk, b = w['gru'][0]
    kp, rp, bp = np.zeros((wr.N_IN, 3 * Hp), np.float32), np.zeros((Hp, 3 * Hp), np.float32), np.zeros(3 * Hp, np.float32)
    for g in range(3):
        kp[:, g * Hp:g * Hp + H] = k[:, g * H:(g + 1) * H]
        rp[:H, g * Hp:g * Hp + H] = rk[:, g * H:(g + 1) * H]
        bp[g * Hp:g * Hp + H] = b[g * H:(g + 1) * H]
    dp = np.zeros((Hp, 1), np.float32)
    dp[:H] = w['dense_kernel']
    wp = {'gru': [(kp, rp, bp)], 'dense_kernel': dp, 'dense_bias': w['dense_bias']}
    x = wr.case_batch((100,))
    a, b_ = engine(w, x.shape[1]), engine(wp, x.shape[1])
    pa, pb = a.predict(x), b_.predict(x)
    a.close(); b_.close()
    assert np.array_equal(bits(pa), bits(pb))
    assert np.array_equal(wr.predict(x, w), wr.predict(x, wp))                    # (and so it is in the contract)


# ---- refusals by name ------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    with pytest.raises(NotImplementedError, match='use_delta'):
        engine(synth.make_weights(n_in=2 * wr.N_IN, units=(64,), seed=900), use_delta=True)
    with pytest.raises(NotImplementedError, match='ring_precision'):
        engine(synth.make_weights(units=(64,), seed=900), ring='bf16')
    with pytest.raises(NotImplementedError, match='ring_precision'):
        engine(synth.make_weights(units=(20, 20), seed=900), ring='bf16')
    eng = engine(synth.make_weights(units=(40, 33), seed=900))
    for tiling in (1, 2):
        with pytest.raises(NotImplementedError, match='one form'):
            eng.set_gru_tiling(tiling)
    assert eng.gru_tiling() == 0
    eng.close()
