"""GPU: many clips of different lengths vectorized / scored in one call (pe_vectorize_clips / pe_score_clips) -- the
dataset tools' path of the reference (train_data.py:195-196: vectorizer(load_audio(x)) per wav; scripts/test.py:48-53,
eval.py:103-105: predict over those vectors) without the per-clip loop.  The main gate is bit-identity to the per-clip
path that already exists (vectorize per clip, then one predict); the oracle bounds the whole thing."""

import numpy as np
import pytest

from mycroft_precise_amd import synth
from mycroft_precise_amd import params as P
from oracle import listener as ol, keras_gru

pytestmark = pytest.mark.gpu

TOL_MFCC = 1e-9         # the project's offline MFCC tolerance (float64 front end against the oracle)
TOL_RAW = 1e-4
TOL_BF16 = 1e-2
MAX_SAMPLES = 24000     # stock params: window 1600, hop 800, T 29
EDGE_LENGTHS = [1, 1599, 1600, 1601, 2399, 2400, 3199, 23999, 24000, 24001, 24799, 24800, 40000]


def make_clips(lengths, first_seed=0):
    return [synth.stream_pcm(first_seed + i, int(n)).astype(np.float64) / 32768.0 for i, n in enumerate(lengths)]


@pytest.fixture(scope='module')
def lengths():
    rng = np.random.default_rng(20240)
    out = EDGE_LENGTHS + [int(v) for v in rng.integers(1, 48001, 54)]
    assert len(out) == 67
    return out


@pytest.fixture(scope='module')
def clips(lengths):
    return make_clips(lengths)


@pytest.fixture(scope='module')
def oracle_vectors(clips):
    """oracle.listener.vectorize of every clip of the standard set (computed once, shared, never written to)"""
    v = np.stack([ol.vectorize(c, ol.Params()) for c in clips])
    v.setflags(write=False)
    return v


def loop_vectorize(eng, clip, max_samples=MAX_SAMPLES, mels=False):
    """vectorization.vectorize (vectorization.py:62-84) on `eng` itself: the per-clip path as it exists without this feature"""
    clip = np.asarray(clip)
    if max_samples > 0 and len(clip) > max_samples:
        clip = clip[-max_samples:]
    feats = eng.vectorize_mels(clip) if mels else eng.vectorize_raw(clip)
    T = eng.n_features
    if len(feats) < T:
        feats = np.concatenate([np.zeros((T - len(feats), feats.shape[1])), feats])
    return feats[-T:]


def engine(weights, n_streams=1, params=None, **kw):
    from mycroft_precise_amd._lib import HipEngine
    return HipEngine(params or P.pr, weights, n_streams=n_streams, **kw)


# ---- 1. bit-identity to the existing path ----------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_clips_equal_the_per_clip_loop_bitwise(stock_weights, clips, prec):
    from mycroft_precise_amd import vectorization as V
    eng = engine(stock_weights, mfcc_precision=prec)
    want = np.stack([loop_vectorize(eng, c) for c in clips])
    if prec == 'f64':
        assert np.array_equal(want, np.stack([V.vectorize(c) for c in clips]))
    clips32 = [c.astype(np.float32) for c in clips]           # (int16 / 32768: exact in float32)
    assert all(np.array_equal(a.astype(np.float64), b) for a, b in zip(clips32, clips))
    for sent in (clips, clips32):
        got = eng.vectorize_clips(sent, MAX_SAMPLES)
        assert got.shape == (67, 29, 13) and got.dtype == np.float64
        assert np.array_equal(got, want)
    for form in (0, 1, 2):
        eng.set_gru_tiling(form)
        assert eng.gru_tiling() == form
        for waves in (1, 4):
            eng.set_gru_waves(waves)
            want_raw = eng.predict(want)
            for sent in (clips, clips32):
                got_raw = eng.score_clips(sent, MAX_SAMPLES)
                assert got_raw.shape == (67, 1) and got_raw.dtype == np.float32
                assert np.array_equal(got_raw, want_raw), (form, waves)
    eng.close()


# ---- 2. parity with the oracle ---------------------------------------------------------------------------------------
def test_clips_match_the_oracle(stock_weights, clips, oracle_vectors):
    eng = engine(stock_weights)
    got = eng.vectorize_clips(clips, MAX_SAMPLES)
    assert got.shape == oracle_vectors.shape
    for c in range(len(clips)):
        assert np.abs(got[c] - oracle_vectors[c]).max() <= TOL_MFCC, c
    raw = eng.score_clips(clips, MAX_SAMPLES)
    want = keras_gru.predict(oracle_vectors, stock_weights)
    assert raw.shape == want.shape == (len(clips), 1)
    assert np.abs(raw.astype(np.float64) - want).max() <= TOL_RAW
    eng.close()


# ---- 3. passes -------------------------------------------------------------------------------------------------------
def test_pass_size_does_not_change_a_bit(stock_weights, clips):
    eng = engine(stock_weights)
    clips32 = [c.astype(np.float32) for c in clips]
    base_v, base_s = eng.vectorize_clips(clips, MAX_SAMPLES), eng.score_clips(clips, MAX_SAMPLES)     # the default target
    for target in (64 << 10, 1, 256 << 20):          # many passes (the 40000-sample clip alone exceeds one); one clip per pass; default
        eng.set_clip_pass_bytes(target)
        for sent in (clips, clips32):
            assert np.array_equal(eng.vectorize_clips(sent, MAX_SAMPLES), base_v), target
            assert np.array_equal(eng.score_clips(sent, MAX_SAMPLES), base_s), target
    with pytest.raises(ValueError):
        eng.set_clip_pass_bytes(0)
    eng.close()


# ---- 4. edges --------------------------------------------------------------------------------------------------------
def test_edges(stock_weights, clips):
    eng = engine(stock_weights)
    # n = 1
    one = eng.vectorize_clips(clips[12:13], MAX_SAMPLES)
    assert one.shape == (1, 29, 13) and np.array_equal(one[0], loop_vectorize(eng, clips[12]))
    assert np.array_equal(eng.score_clips(clips[12:13], MAX_SAMPLES), eng.predict(one))
    # n = 0: an empty result and no launch
    eng.set_timing(True)
    assert eng.vectorize_clips([], MAX_SAMPLES).shape == (0, 29, 13)
    assert eng.score_clips([], MAX_SAMPLES).shape == (0, 1)
    with pytest.raises(ValueError):
        eng.last_timing()                             # nothing was timed: nothing was launched
    eng.set_timing(False)
    # all clips shorter than a window: all-zero windows, the score of a zero window
    short = make_clips([1, 7, 800, 1599, 1599, 1000])
    assert np.array_equal(eng.vectorize_clips(short, MAX_SAMPLES), np.zeros((6, 29, 13)))
    assert np.array_equal(eng.score_clips(short, MAX_SAMPLES), eng.predict(np.zeros((6, 29, 13), np.float32)))
    # max_samples <= 0: no crop -- a 40000-sample clip keeps the last 29 of its 49 frames
    for ms in (0, -1):
        full = eng.vectorize_clips([clips[12]], ms)
        raw = eng.vectorize_raw(clips[12])
        assert len(raw) == 49 and np.array_equal(full[0], raw[-29:])
        # (40000 - 24000 is a whole number of hops, so the crop keeps those same frames; it moves the anchor of a
        # 24001-sample clip by one sample, and then every frame differs)
        assert np.array_equal(full, one)
        odd = eng.vectorize_clips([clips[9]], ms)
        assert np.array_equal(odd[0], eng.vectorize_raw(clips[9])[-29:])
        assert np.array_equal(eng.vectorize_clips([clips[9]], MAX_SAMPLES)[0], eng.vectorize_raw(clips[9][1:]))
        assert np.all(np.any(odd != eng.vectorize_clips([clips[9]], MAX_SAMPLES), axis=-1))
    # an empty clip in the middle of the batch: refused before anything is written
    bad = clips[:3] + [np.zeros(0)] + clips[3:6]
    out_v = np.full((7, 29, 13), 7.25)
    with pytest.raises(ValueError, match='clip 3'):
        eng.vectorize_clips(bad, MAX_SAMPLES, out=out_v)
    assert np.all(out_v == 7.25)
    out_s = np.full((7, 1), 7.25, np.float32)
    with pytest.raises(ValueError, match='clip 3'):
        eng.score_clips(bad, MAX_SAMPLES, out=out_s)
    assert np.all(out_s == 7.25)
    # decreasing offsets (the C ABI directly), a bad sample format, null pointers, n_clips < 0
    audio = np.concatenate(clips[:2])
    offsets = np.array([0, len(audio), len(clips[0])], dtype=np.int64)
    for off, fmt, n, a in ((offsets, 0, 2, audio), (np.array([0, 5, 9], np.int64), 2, 2, audio), (np.array([0, 5, 9], np.int64), 0, -1, audio),
                           (np.array([1, 5, 9], np.int64), 0, 2, audio), (np.array([0, 5, 9], np.int64), 0, 2, None)):
        rc = eng._lib.pe_vectorize_clips(eng._h, a.ctypes.data if a is not None else None, fmt, off.ctypes.data, n, MAX_SAMPLES, 0, out_v.ctypes.data)
        with pytest.raises(ValueError):
            eng._check(rc)
        rc = eng._lib.pe_score_clips(eng._h, a.ctypes.data if a is not None else None, fmt, off.ctypes.data, n, MAX_SAMPLES, out_s.ctypes.data)
        with pytest.raises(ValueError):
            eng._check(rc)
    assert np.all(out_v == 7.25) and np.all(out_s == 7.25)
    eng.close()


# ---- 5. other configurations (n = 19, lengths from the standard set) ------------------------------------------------
N19 = EDGE_LENGTHS + [31337, 5000, 47999, 12345, 801, 16000]


def test_speechpy_front_end_one_frame_fewer(stock_weights):
    opr = ol.Params(vectorizer=3)
    hpr = P.pr.copy()
    hpr.__dict__['vectorizer'] = P.Vectorizer.speechpy_mfccs
    clips = make_clips(N19, 100)
    eng = engine(stock_weights, params=hpr)
    got = eng.vectorize_clips(clips, MAX_SAMPLES)
    want = np.stack([ol.vectorize(c, opr) for c in clips])
    assert np.abs(got - want).max() <= TOL_MFCC
    assert np.all(got[2] == 0) and np.all(got[4] == 0) and np.any(got[5][-1] != 0)     # 1600 / 2399 samples: no frame yet; 2400: one
    assert np.all(got[8][0] == 0) and np.any(got[8][1] != 0)                          # 24000 samples: 28 frames, one pad row
    assert np.array_equal(got, np.stack([loop_vectorize(eng, c) for c in clips]))
    assert np.abs(eng.score_clips(clips, MAX_SAMPLES) - keras_gru.predict(want, stock_weights)).max() <= TOL_RAW
    eng.close()


def test_mels_rows(stock_weights):
    from mycroft_precise_amd import vectorization as V
    clips = make_clips(N19, 200)
    saved = P.pr.vectorizer
    try:
        P.pr.__dict__['vectorizer'] = P.Vectorizer.mels
        want = np.stack([V.vectorize(c) for c in clips])
        assert want.shape == (19, 29, 20)
        assert np.array_equal(V.vectorize_batch(clips), want)
    finally:
        P.pr.__dict__['vectorizer'] = saved
    eng = engine(stock_weights)
    assert np.array_equal(eng.vectorize_clips(clips, MAX_SAMPLES, mels=True), want)
    eng.close()


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_general_front_end(prec):
    """one parameter set of test_general_listener_params_offline (n_fft = 1024, 40 filters, 20 coefficients: 32-float rows),
    and -- float64 -- the Bluestein form (n_fft = 400)"""
    import warnings
    from oracle import sonopy_restated as sr
    for kw in ([dict(n_fft=1024, n_filt=40, n_mfcc=20), dict(n_fft=400, n_filt=26, n_mfcc=13)] if prec == 'f64' else [dict(n_fft=1024, n_filt=40, n_mfcc=20)]):
        opr = ol.Params(**kw)
        hpr = P.pr.copy()
        hpr.__dict__.update(kw)
        w = synth.make_weights(n_in=kw['n_mfcc'], units=(8,), seed=3)
        clips = make_clips(N19, 300)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            eng = engine(w, params=hpr, mfcc_precision=prec)
        got = eng.vectorize_clips(clips, MAX_SAMPLES)
        want = np.stack([loop_vectorize(eng, c) for c in clips])
        assert got.shape == (19, 29, kw['n_mfcc']) and np.array_equal(got, want)
        assert np.array_equal(eng.vectorize_clips([c.astype(np.float32) for c in clips], MAX_SAMPLES), want)
        assert np.array_equal(eng.vectorize_clips(clips, MAX_SAMPLES, mels=True), np.stack([loop_vectorize(eng, c, mels=True) for c in clips]))
        assert np.array_equal(eng.score_clips(clips, MAX_SAMPLES), eng.predict(want))
        if prec == 'f64':
            ref = np.stack([ol.vectorize(c, opr) for c in clips])
            assert np.abs(got - ref).max() <= TOL_MFCC
            assert np.abs(eng.score_clips(clips, MAX_SAMPLES) - keras_gru.predict(ref, w)).max() <= TOL_RAW
        eng.close()


def delta_case():
    """19 clips; clip 7 ends in full-scale audio and clip 8 is short (3 frames behind 26 pad rows), clip 9 ends loud and clip
    10 has no frame at all: a first-row delta that leaked from the previous clip's last row would be enormous there"""
    clips = make_clips(N19, 400)
    clips[7] = synth.stream_pcm(7, 30000, 'square').astype(np.float64) / 32768.0
    clips[8] = synth.stream_pcm(8, 3300, 'quiet').astype(np.float64) / 32768.0
    clips[9] = synth.stream_pcm(9, 24000, 'square').astype(np.float64) / 32768.0
    clips[10] = synth.stream_pcm(10, 900, 'quiet').astype(np.float64) / 32768.0
    return clips


@pytest.mark.parametrize('tiling,gru,ring', [(0, 'f32', 'f32'), (1, 'f32', 'f32'), (-1, 'bf16', 'f32'), (0, 'bf16', 'f32'), (-1, 'bf16', 'bf16')])
def test_use_delta_windows_start_with_zero_deltas(tiling, gru, ring):
    w = synth.make_weights(n_in=26, units=(20,), seed=77)
    k, rk, b = w['gru'][0]
    b = b.copy()
    b[:20] += np.float32(2.4)          # update gates near 1: the state keeps what the FIRST timestep did to it until the last one
    w['gru'] = [(k, rk, b)]
    opr = ol.Params(use_delta=True)
    hpr = P.pr.copy()
    hpr.__dict__['use_delta'] = True
    clips = delta_case()
    x = np.stack([ol.add_deltas(ol.vectorize(c, opr)) for c in clips])
    assert x.shape == (19, 29, 26)
    want = keras_gru.predict(x, w)
    # what a leak would do: the delta of the first row taken against the previous clip's last row
    leaky = x.copy()
    for c in range(1, 19):
        leaky[c, 0, 13:] = x[c, 0, :13] - x[c - 1, -1, :13]
    assert np.abs(keras_gru.predict(leaky, w) - want)[[8, 10]].min() > max(10 * TOL_RAW, 2 * TOL_BF16)     # (0.026 and 0.032)
    eng = engine(w, params=hpr, gru_precision=gru, ring_precision=ring)
    eng.set_gru_tiling(tiling)
    got = eng.score_clips(clips, MAX_SAMPLES)
    assert np.abs(got - want).max() <= (TOL_RAW if gru == 'f32' else TOL_BF16)
    # every clip alone gives the same bits: nothing of a window depends on its neighbours
    assert np.array_equal(got, np.concatenate([eng.score_clips([c], MAX_SAMPLES) for c in clips]))
    eng.close()


@pytest.mark.parametrize('ring', ['f32', 'bf16'])
def test_bf16_network(stock_weights, ring):
    clips = make_clips(N19, 500)
    want = keras_gru.predict(np.stack([ol.vectorize(c, ol.Params()) for c in clips]), stock_weights)
    eng = engine(stock_weights, gru_precision='bf16', ring_precision=ring)
    for tiling in (-1, 0):
        eng.set_gru_tiling(tiling)
        assert np.abs(eng.score_clips(clips, MAX_SAMPLES) - want).max() <= TOL_BF16
    eng.close()


def test_three_models_share_the_front_end(stock_weights):
    clips = make_clips(N19, 600)
    ws = [stock_weights, synth.make_weights(seed=5), synth.make_weights(seed=6)]
    multi = engine(ws)
    got = multi.score_clips(clips, MAX_SAMPLES)
    assert got.shape == (3, 19, 1)
    multi.set_clip_pass_bytes(100000)                # K models across passes: every model's block in its place
    assert np.array_equal(multi.score_clips(clips, MAX_SAMPLES), got)
    for m, w in enumerate(ws):
        single = engine(w)
        assert np.array_equal(got[m], single.score_clips(clips, MAX_SAMPLES)), m
        single.close()
    multi.close()


@pytest.mark.parametrize('tiling', [0, 2])
def test_wide_network(tiling):
    w = synth.make_weights(units=(64, 64), seed=564)
    clips = make_clips(N19, 700)
    want = keras_gru.predict(np.stack([ol.vectorize(c, ol.Params()) for c in clips]), w)
    eng = engine(w)
    eng.set_gru_tiling(tiling)
    assert np.abs(eng.score_clips(clips, MAX_SAMPLES) - want).max() <= TOL_RAW
    eng.close()


# ---- 6. statelessness ------------------------------------------------------------------------------------------------
def test_streams_are_untouched(stock_weights, clips):
    n = 19
    pcm = synth.batch_pcm(n, 12, 1024)
    a, b = engine(stock_weights, n_streams=n), engine(stock_weights, n_streams=n)
    for u in range(12):
        ra = a.update(pcm[u])
        if u in (3, 7):
            state = a.stream_state()
            a.score_clips(clips[:20], MAX_SAMPLES)
            a.vectorize_clips(clips[:20], MAX_SAMPLES)
            assert all(np.array_equal(x, y) for x, y in zip(state, a.stream_state()))
        if u == 5:                                    # ... and behind an update still in flight
            a.wait()
        assert np.array_equal(ra, b.update(pcm[u])), u
    out = a.update_async(pcm[0])
    a.score_clips(clips[:5], MAX_SAMPLES)             # drains the update in flight first
    assert np.array_equal(out, b.update(pcm[0]))
    assert np.array_equal(a.get_vectors(), b.get_vectors())
    a.close(); b.close()


# ---- Python surface --------------------------------------------------------------------------------------------------
def test_vectorize_batch_and_predict_clips(stock_weights, clips):
    from mycroft_precise_amd import vectorization as V
    from mycroft_precise_amd.network_runner import HipRunner
    from mycroft_precise_amd.util import InvalidAudio
    sub = clips[:19]
    want = np.stack([V.vectorize(c) for c in sub])
    assert np.array_equal(V.vectorize_batch(sub), want)
    runner = HipRunner(weights=stock_weights)
    assert np.array_equal(runner.predict_clips(sub), runner.predict(want))
    with pytest.raises(InvalidAudio):
        runner.predict_clips(sub[:2] + [np.zeros(0)])
    saved = dict(P.pr.__dict__)
    try:
        P.pr.__dict__['use_delta'] = True
        assert np.array_equal(V.vectorize_batch(sub), np.stack([V.vectorize_delta(c) for c in sub]))
        w = synth.make_weights(n_in=26, units=(20,), seed=77)
        delta_runner = HipRunner(weights=w)
        x = np.stack([V.vectorize_delta(c) for c in sub])
        assert np.abs(delta_runner.predict_clips(sub) - delta_runner.predict(x)).max() <= TOL_RAW  # (float32 deltas in registers against float64 deltas rounded once)
        P.pr.__dict__['use_delta'] = False
        P.pr.__dict__['vectorizer'] = P.Vectorizer.speechpy_mfccs
        assert np.array_equal(V.vectorize_batch(sub), np.stack([V.vectorize(c) for c in sub]))
    finally:
        P.pr.__dict__.clear()
        P.pr.__dict__.update(saved)


def test_vectorize_batch_follows_buffer_t(clips):
    """pr.buffer_t sets n_features and max_samples; it may change between two calls (a model loaded with other params), and
    the batch then has the new window length, as the per-clip function does"""
    from mycroft_precise_amd import vectorization as V
    sub = clips[:19]
    saved = dict(P.pr.__dict__)
    try:
        for buffer_t, T in ((1.5, 29), (1.0, 19), (2.0, 39), (1.5, 29)):
            P.pr.__dict__['buffer_t'] = buffer_t
            assert P.pr.n_features == T
            want = np.stack([V.vectorize(c) for c in sub])
            got = V.vectorize_batch(sub)
            assert got.shape == want.shape == (19, T, 13)
            assert np.array_equal(got, want), buffer_t
    finally:
        P.pr.__dict__.clear()
        P.pr.__dict__.update(saved)
