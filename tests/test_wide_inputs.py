"""
-m gpu: float32 wide / stacked networks (33..256 units, one or two layers; csrc/gru_wide_device.h and gru_wide_x3_device.h,
forms 0 and 2) on up to 32 inputs per frame -- use_delta over <= 16 coefficients (the second 16-input k-group is
x_t - x_(t-1), formed in the kernel, zero at timestep 0 of every window) and 17..32 coefficients (32-float rows).

Bar: TOL_RAW = 1e-4 against oracle.keras_gru / oracle.listener; every test prints its worst distance before it asserts
(DESIGN.md 4.4 records them).  Bit-for-bit checks tie the entry points to each other and the new instantiations to the
one-group kernels.
"""
import faulthandler
import warnings

import numpy as np
import pytest

from mycroft_precise_amd import params as P
from mycroft_precise_amd import synth
from oracle import keras_gru
from oracle import listener as ol

pytestmark = pytest.mark.gpu

TOL_RAW = 1e-4
TIME_LIMIT_S = 120              # per test: a hung launch ends the whole run instead of the next test starting on the card
FORMS = [0, 2]
FORM_IDS = ['f32mfma', 'xdl']

DELTA = dict(use_delta=True)                                    # 2 x 13 inputs
DELTA16 = dict(use_delta=True, n_mfcc=16)                       # 2 x 16: both groups full
COEF17 = dict(n_fft=1024, n_filt=40, n_mfcc=17)                 # the first column beyond one 16-float row
COEF20 = dict(n_fft=1024, n_filt=40, n_mfcc=20)
COEF32 = dict(n_fft=1024, n_filt=40, n_mfcc=32)


@pytest.fixture(autouse=True)
def time_limit_and_params():
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    saved = dict(P.pr.__dict__)
    yield
    P.pr.__dict__.clear()
    P.pr.__dict__.update(saved)
    faulthandler.cancel_dump_traceback_later()


def params(**kw):
    hpr = P.pr.copy()
    hpr.__dict__.update(kw)
    return hpr


def engine(weights, kw, n_streams=1, tiling=0, **ekw):
    from mycroft_precise_amd._lib import HipEngine
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')              # (UnverifiedFilterbank for colliding mel grids: flagged, still served)
        eng = HipEngine(params(**kw), weights, n_streams=n_streams, **ekw)
    eng.set_gru_tiling(tiling)
    assert eng.gru_tiling() == tiling
    return eng


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def stream_batch(kinds, n_up, chunk=1024):
    return np.stack([synth.stream_pcm(s, n_up * chunk, k).reshape(n_up, chunk) for s, k in enumerate(kinds)], axis=1)


def with_deltas32(x):
    """[n, T, F] float32 -> [n, T, 2 F]: the delta columns as the kernel forms them (float32, zero first row)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    d = np.zeros_like(x)
    d[:, 1:] = x[:, 1:] - x[:, :-1]
    return np.concatenate([x, d], axis=2)


_want = {}


def oracle_predict(key, x, w):
    """keras_gru.predict, once per case (the two forms share it)"""
    if key not in _want:
        _want[key] = keras_gru.predict(x, w)
    return _want[key]


# ---- 1. explicit batches by width and form -----------------------------------------------------------------------------
WIDTHS = [(33,), (64,), (100,), (256,), (40, 33), (256, 256)]
BATCH_CASES = [(u, n_in, kw) for u in WIDTHS for n_in, kw in ((26, DELTA), (20, COEF20))] + \
              [(u, n_in, kw) for u in [(33,), (256, 256)] for n_in, kw in ((32, DELTA16), (17, COEF17), (32, COEF32))]


def batch_id(case):
    units, n_in, kw = case
    return '%s-%s%d' % ('x'.join(str(u) for u in units), 'delta' if kw.get('use_delta') else 'in', n_in)


@pytest.mark.parametrize('tiling', FORMS, ids=FORM_IDS)
@pytest.mark.parametrize('case', BATCH_CASES, ids=batch_id)
def test_predict_by_width_and_form(case, tiling):
    units, n_in, kw = case
    assert params(**kw).feature_size == n_in
    w = synth.make_weights(n_in=n_in, units=units, seed=700 + sum(units) + n_in)
    x = np.random.default_rng(n_in + len(units)).normal(0, 2, (37, 29, n_in)).astype(np.float32)
    want = oracle_predict(batch_id(case), x, w)
    eng = engine(w, kw, tiling=tiling)
    worst = 0.0
    for n in (1, 17, 37):
        got = eng.predict(x[:n])
        assert got.shape == (n, 1)
        worst = max(worst, float(np.abs(got - want[:n]).max()))
    eng.close()
    print('predict %-16s form %d: worst %.3g' % (batch_id(case), tiling, worst))
    assert worst <= TOL_RAW, (batch_id(case), tiling, worst)


# ---- 2. / 3. streaming: ring mode, masked clear, a ring that wraps; then the offline evaluator (row sequences) ----------------
def streaming_case(label, w, kw, n, tiling, delta):
    from mycroft_precise_amd.network_runner import BatchedListener, HipRunner
    from oracle import sonopy_restated as so
    opr, hpr = ol.Params(**kw), params(**kw)
    n_up = 36                                        # 36 updates of 1-2 frames wrap the 32-slot ring
    kinds = ['tone_noise'] * (n - 3) + ['zeros', 'square', 'quiet']
    pcm = stream_batch(kinds, n_up)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        hip = BatchedListener(w, n, params=hpr)
    hip.engine.set_gru_tiling(tiling)
    assert hip.engine.info().ring_slots == 32
    refs = [ol.OracleListener(w, opr) for _ in range(n)]
    worst = 0.0
    for u in range(n_up):
        if u == 20:
            mask = np.zeros(n, np.uint8); mask[::4] = 1
            hip.clear(mask)
            for j in np.nonzero(mask)[0]:
                refs[j].clear()
        raw = hip.update_raw(pcm[u])
        want = np.array([r.update_raw(pcm[u, j].tobytes()) for j, r in enumerate(refs)])
        worst = max(worst, float(np.abs(raw - want).max()))
    hip.engine.close()
    print('%s form %d: streaming worst %.3g' % (label, tiling, worst))
    assert worst <= TOL_RAW, (label, worst)
    # the offline evaluator on one 4 s recording: windows of the row sequence, deltas inside each window
    P.pr.__dict__.update(kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        runner = HipRunner(weights=w)
    runner.engine.set_gru_tiling(tiling)
    audio = synth.stream_pcm(9, 16000 * 4).astype(np.float32) / np.float32(32768.0)
    got = runner.evaluate(audio, 2048)
    runner.engine.close()
    mf = so.mfcc_spec(audio.astype(np.float64), opr.sample_rate, (opr.window_samples, opr.hop_samples), opr.n_fft, opr.n_filt, opr.n_mfcc)
    T = opr.n_features
    win = [mf[i - T:i] for i in range(T, len(mf), 2)]
    win = np.stack([ol.add_deltas(m) for m in win]) if delta else np.stack(win)
    want = keras_gru.predict(win, w)
    far = float(np.abs(got - want).max())
    print('%s form %d: evaluate worst %.3g over %d windows' % (label, tiling, far, len(win)))
    assert got.shape == want.shape and far <= TOL_RAW, (label, far)


@pytest.mark.parametrize('tiling', FORMS, ids=FORM_IDS)
def test_streaming_with_use_delta(tiling):
    w = synth.make_weights(n_in=26, units=(128, 100), seed=811)
    streaming_case('delta 128x100', w, DELTA, 21, tiling, True)


@pytest.mark.parametrize('units', [(64,), (72, 200)], ids=['64', '72x200'])
@pytest.mark.parametrize('tiling', FORMS, ids=FORM_IDS)
def test_streaming_with_20_coefficients(units, tiling):
    w = synth.make_weights(n_in=20, units=units, seed=812 + sum(units))
    streaming_case('20 coefficients %s' % 'x'.join(str(u) for u in units), w, COEF20, 12, tiling, False)


# ---- 4. one engine, every path, same bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize('tiling', FORMS, ids=FORM_IDS)
def test_every_path_gives_the_same_bits(tiling):
    n = 37
    w = synth.make_weights(n_in=26, units=(40, 33), seed=821)
    w2 = synth.make_weights(n_in=26, units=(40, 33), seed=822)
    pcm = stream_batch(['tone_noise'] * (n - 2) + ['zeros', 'square'], 36)
    base = engine(w, DELTA, n, tiling)
    outs = [base.update(pcm[u]) for u in range(36)]
    assert len({o.tobytes() for o in outs[30:]}) > 1
    # update_many of 6 == six updates
    many = engine(w, DELTA, n, tiling)
    many.reserve_updates(6, 1024)
    for u in range(0, 36, 6):
        assert np.array_equal(bits(many.update_many(pcm[u:u + 6])), bits(np.stack(outs[u:u + 6]))), u
    many.close()
    # update_subset over all ids in shuffled order == update, permuted
    sub = engine(w, DELTA, n, tiling)
    rng = np.random.default_rng(4)
    for u in range(36):
        ids = rng.permutation(n).astype(np.int32)
        assert np.array_equal(bits(sub.update_subset(ids, pcm[u][ids])), bits(outs[u][ids])), u
    sub.close()
    # two models in one engine == two engines; set_weights(w2) == a fresh engine on w2
    other = engine(w2, DELTA, n, tiling)
    outs2 = [other.update(pcm[u]) for u in range(36)]
    other.close()
    both = engine([w, w2], DELTA, n, tiling)
    for u in range(36):
        got = both.update(pcm[u])
        assert got.shape == (2, n)
        assert np.array_equal(bits(got[0]), bits(outs[u])) and np.array_equal(bits(got[1]), bits(outs2[u])), u
    both.close()
    swapped = engine(w, DELTA, n, tiling)
    for u in range(18):
        assert np.array_equal(bits(swapped.update(pcm[u])), bits(outs[u])), u
    swapped.set_weights(w2)
    for u in range(18, 36):
        assert np.array_equal(bits(swapped.update(pcm[u])), bits(outs2[u])), u
    swapped.close()
    # ring mode and explicit mode feed the same float32 operands in the same order: predict on the windows the last update
    # read, with float32 deltas, IS that update
    x = base.get_vectors()
    assert x.shape == (n, 29, 13) and x.dtype == np.float32
    batch = with_deltas32(x)
    assert np.array_equal(bits(base.predict(batch)[:, 0]), bits(outs[-1]))
    # ... and within TOL_RAW of the oracle on float64 add_deltas
    want = keras_gru.predict(np.stack([ol.add_deltas(v.astype(np.float64)) for v in x]), w)[:, 0]
    worst = float(np.abs(outs[-1] - want).max())
    print('form %d: last update against the oracle over add_deltas: %.3g' % (tiling, worst))
    assert worst <= TOL_RAW
    base.close()


# ---- 5. the second group is inert where its weights are zero ---------------------------------------------------------------------
@pytest.mark.parametrize('tiling', FORMS, ids=FORM_IDS)
@pytest.mark.parametrize('units', [(64,), (40, 33), (256,)], ids=['64', '40x33', '256'])
def test_second_group_with_zero_weights_is_inert(units, tiling):
    rng = np.random.default_rng(5)
    # delta network, kernel rows F .. 2F-1 zero, arbitrary finite delta columns == the plain 13-input network
    w = synth.make_weights(n_in=26, units=units, seed=831)
    k, rk, b = w['gru'][0]
    k = k.copy(); k[13:] = 0
    w['gru'] = [(k, rk, b)] + list(w['gru'][1:])
    w13 = dict(w, gru=[(k[:13].copy(), rk, b)] + list(w['gru'][1:]))
    x = rng.normal(0, 2, (37, 29, 26)).astype(np.float32)
    x[:, :, 13:] *= 50
    a, p = engine(w, DELTA, tiling=tiling), engine(w13, {}, tiling=tiling)
    got, plain = a.predict(x), p.predict(np.ascontiguousarray(x[:, :, :13]))
    a.close(); p.close()
    assert np.array_equal(bits(got), bits(plain))
    # 20 inputs, kernel rows 16 .. 19 zero == the 16-input network on x[..., :16]
    w = synth.make_weights(n_in=20, units=units, seed=832)
    k, rk, b = w['gru'][0]
    k = k.copy(); k[16:] = 0
    w['gru'] = [(k, rk, b)] + list(w['gru'][1:])
    w16 = dict(w, gru=[(k[:16].copy(), rk, b)] + list(w['gru'][1:]))
    x = rng.normal(0, 2, (37, 29, 20)).astype(np.float32)
    x[:, :, 16:] *= 50
    a, p = engine(w, COEF20, tiling=tiling), engine(w16, dict(n_mfcc=16), tiling=tiling)
    got, plain = a.predict(x), p.predict(np.ascontiguousarray(x[:, :, :16]))
    a.close(); p.close()
    assert np.array_equal(bits(got), bits(plain))


# ---- 6. streams do not leak ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tiling', FORMS, ids=FORM_IDS)
def test_an_infinite_feature_stays_in_its_window(tiling):
    w = synth.make_weights(n_in=26, units=(64,), seed=841)
    x = np.random.default_rng(6).normal(0, 2, (17, 29, 26)).astype(np.float32)
    eng = engine(w, DELTA, tiling=tiling)
    clean = eng.predict(x)[:, 0]
    bad = x.copy()
    bad[5, 10, 20] = np.inf
    got = eng.predict(bad)[:, 0]
    eng.close()
    others = np.arange(17) != 5
    assert np.all(np.isfinite(clean))
    assert np.array_equal(bits(got[others]), bits(clean[others]))


# ---- 7. clips -------------------------------------------------------------------------------------------------------------------
def test_predict_clips_with_use_delta():
    from mycroft_precise_amd.network_runner import HipRunner
    opr = ol.Params(use_delta=True)
    P.pr.__dict__['use_delta'] = True
    w = synth.make_weights(n_in=26, units=(64,), seed=851)
    lengths = [24000, 900, 31234, 16000, 40000]              # 900 samples: shorter than a window
    clips = [synth.stream_pcm(60 + i, m, 'tone_noise' if i != 3 else 'square').astype(np.float64) / 32768.0 for i, m in enumerate(lengths)]
    want = keras_gru.predict(np.stack([ol.add_deltas(ol.vectorize(c, opr)) for c in clips]), w)
    runner = HipRunner(weights=w)
    for tiling in FORMS:
        runner.engine.set_gru_tiling(tiling)
        got = runner.predict_clips(clips)
        worst = float(np.abs(got - want).max())
        print('predict_clips form %d: worst %.3g' % (tiling, worst))
        assert got.shape == want.shape and worst <= TOL_RAW, (tiling, worst)
    runner.engine.close()


# ---- 8. train, save, serve: the loop this exists for ------------------------------------------------------------------------------
@pytest.mark.parametrize('units', [64, (40, 33)], ids=['64', '40x33'])
def test_train_save_serve_with_use_delta(tmp_path, units):
    from mycroft_precise_amd.model import ModelParams, load_weights
    from mycroft_precise_amd.network_runner import HipRunner, Listener
    from mycroft_precise_amd.train import Trainer
    P.pr.__dict__['use_delta'] = True
    assert P.pr.feature_size == 26
    rng = np.random.default_rng(8)
    x = rng.normal(0, 1, (40, 29, 26)).astype(np.float32)
    y = (rng.random((40, 1)) < 0.5).astype(np.float64)
    path = str(tmp_path / 'delta_wide.npz')
    tr = Trainer(params=ModelParams(recurrent_units=units), seed=3)
    try:
        tr.fit(x, y, batch_size=20, epochs=2)
        tr.save(path)
        w = tr.weights
    finally:
        tr.close()
    assert np.shape(load_weights(path)['gru'][0][0])[0] == 26
    runner = HipRunner(path)
    got, want = runner.predict(x), keras_gru.predict(x, w)
    runner.engine.close()
    worst = float(np.abs(got - want).max())
    print('trained %s: HipRunner.predict worst %.3g' % (units, worst))
    assert got.shape == want.shape and worst <= TOL_RAW
    P.pr.__dict__['use_delta'] = False                   # the saved .params, not the process's state, says use_delta
    lis = Listener(path, 2048)
    assert lis.pr.use_delta is True
    ref = ol.OracleListener(w, ol.Params(use_delta=True))
    data = synth.stream_pcm(3, 12 * 1024).tobytes()
    far = 0.0
    for off in range(0, len(data), 2048):
        far = max(far, abs(lis.update_raw(data[off:off + 2048]) - ref.update_raw(data[off:off + 2048])))
    print('trained %s: Listener worst %.3g over 12 updates' % (units, far))
    assert far <= TOL_RAW


# ---- 9. what stays refused, by name -------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    with pytest.raises(NotImplementedError, match=r'use_delta over more than 16 coefficients \(n_mfcc = 17: 34 inputs'):
        engine(synth.make_weights(n_in=34, units=(64,), seed=41), dict(COEF17, use_delta=True))
    with pytest.raises(NotImplementedError, match='use_delta has no bf16-operand wide-GRU kernel'):
        engine(synth.make_weights(n_in=26, units=(64,), seed=41), DELTA, gru_precision='bf16')
    with pytest.raises(NotImplementedError, match=r'more than 16 coefficients per frame \(n_mfcc = 20\) have no bf16-operand wide-GRU kernel'):
        engine(synth.make_weights(n_in=20, units=(72, 200), seed=41), COEF20, gru_precision='bf16')
