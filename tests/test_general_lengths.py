"""GPU: every transform instantiation of the general front end (csrc/mfcc_general_device.h; the table and the dispatch
restatement are in tests/general_lengths_common.py) against the oracle, in float64 AND float32, through each of its four
kernels: offline (vectorize_raw / vectorize_mels), streaming (update / update_subset), clips (vectorize_clips) and recordings
(evaluate_clips).

Bars.  float64: the project's offline 1e-9 on features and log-mel rows, TOL_FEAT32 on the float32 ring rows, GUARD_RAW on
probabilities.  float32: the hard caps the stock float32 front end is held to (2e-4 on features, TOL_RAW on probabilities),
and a guard measured at run time: the float32 restatement of the oracle (general_lengths_common.float32_restatement) is this
far from the float64 oracle on the SAME frames, and the kernel gets 8 x that -- a radix-2 transform has up to 11 rounding
stages where pocketfft's mixed radix has about half, Bluestein runs three transforms and two pointwise products, and the
kernel fuses multiplies and adds in another order.  Every figure is printed before it is asserted (pytest -s);
profiles/general_lengths/README.md holds the table measured on an MI355X."""
import warnings

import numpy as np
import pytest

import general_lengths_common as G
from mycroft_precise_amd import synth
from mycroft_precise_amd import params as P
from oracle import listener as ol, keras_gru
from oracle import sonopy_restated as sr

pytestmark = pytest.mark.gpu

TOL_MFCC = 1e-9         # float64 front end against the oracle, offline
TOL_FEAT32 = 2e-5       # float32 rounding of |feature| <= 40 (ring rows)
GUARD_RAW = 2e-5        # probabilities behind the float64 front end
TOL_RAW = 1e-4          # probabilities behind the float32 front end
CAP_FEAT_F32 = 2e-4     # features of the float32 front end (test_gpu_parity.py: test_batched_streams_match_oracle)
GUARD_X = 8.0           # float32 kernel error <= GUARD_X * the float32 restatement's error on the same frames

PRECS = ['f64', 'f32']
N_UPDATES = 24
SUBSET_AT = 11          # the update that goes through update_subset


def engine(kw, weights, n_streams=1, prec='f64'):
    from mycroft_precise_amd._lib import HipEngine
    from mycroft_precise_amd import vectorization as V
    hpr = P.pr.copy()
    hpr.__dict__.update(kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', V.UnverifiedFilterbank)           # (colliding mel grids at most small lengths: flagged, still served)
        return HipEngine(hpr, weights, n_streams=n_streams, mfcc_precision=prec)


def weights_of(kw):
    return synth.make_weights(n_in=kw['n_mfcc'], units=(8,), seed=3)


def win_hop(opr):
    return opr.window_samples, opr.hop_samples


def err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) if np.size(want) else 0.0


def hold(kw, prec, kernel, what, kernel_err, restated_err, tol64, cap32):
    """print the figures, then assert the bar of the precision"""
    print('GENLEN | %s | %s | %s | %s | %.3g | %s |' % (G.set_id(kw), prec, kernel, what, kernel_err,
                                                         '-' if restated_err is None else '%.3g' % restated_err))
    if prec == 'f64':
        assert kernel_err <= tol64, (what, kernel_err)
    else:
        assert kernel_err <= cap32, (what, kernel_err)
        if restated_err is not None:
            assert kernel_err <= GUARD_X * restated_err, (what, kernel_err, restated_err)


def frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


_CACHE = {}


def shared(key, make):
    """a reference is computed once per parameter set, shared by both precisions, never written to"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def restated(frames, opr):
    return G.float32_restatement(frames, opr.n_fft, opr.n_filt, opr.n_mfcc, opr.sample_rate, with_mels=True)


# ---- 1. offline kernel ---------------------------------------------------------------------------------------------------
def offline_reference(kw):
    def make():
        opr = ol.Params(**kw)
        rows, r32, r32_mels = [], 0.0, 0.0
        for kind, audio in G.offline_inputs(kw['n_fft']):
            _, _, mels, mfcc = sr.mfcc_spec(audio, opr.sample_rate, win_hop(opr), opr.n_fft, opr.n_filt, opr.n_mfcc, return_parts=True)
            m32, l32 = restated(G.frames_of(audio, *win_hop(opr)), opr)
            r32, r32_mels = max(r32, err(m32, mfcc)), max(r32_mels, err(l32, mels))
            rows.append((kind, frozen(audio), frozen(mfcc), frozen(mels)))
        return rows, r32, r32_mels
    return shared(('offline', G.set_id(kw)), make)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('kw', G.LENGTHS, ids=G.set_id)
def test_offline_kernel(kw, prec):
    rows, r32, r32_mels = offline_reference(kw)
    eng = engine(kw, weights_of(kw), prec=prec)
    worst = worst_mels = 0.0
    for kind, audio, mfcc, mels in rows:
        got, got_mels = eng.vectorize_raw(audio), eng.vectorize_mels(audio)
        assert got.shape == mfcc.shape and got.shape[1] == kw['n_mfcc'] and got_mels.shape == mels.shape, kind
        assert np.isfinite(got).all() and np.isfinite(got_mels).all(), kind
        worst, worst_mels = max(worst, err(got, mfcc)), max(worst_mels, err(got_mels, mels))
    eng.close()
    hold(kw, prec, 'offline', 'features', worst, r32, TOL_MFCC, CAP_FEAT_F32)
    hold(kw, prec, 'offline', 'mels', worst_mels, r32_mels, TOL_MFCC, CAP_FEAT_F32)


# ---- 2. streaming kernel -------------------------------------------------------------------------------------------------
def stream_reference(kw, chunk):
    """one stream per input kind, N_UPDATES chunks: the oracle's raw output after every update, its feature rows at the end,
    and how far the float32 restatement of those rows is from them"""
    def make():
        opr = ol.Params(**kw)
        kinds = G.stream_kinds(kw['n_fft'])
        pcm = np.stack([synth.stream_pcm(s, N_UPDATES * chunk, k).reshape(N_UPDATES, chunk) for s, k in kinds], axis=1)
        refs = [ol.OracleListener(weights_of(kw), opr) for _ in kinds]
        raw = np.array([[r.update_raw(pcm[u, j].tobytes()) for j, r in enumerate(refs)] for u in range(N_UPDATES)])
        feats = np.stack([r.mfccs for r in refs])
        T, r32 = opr.n_features, 0.0
        for j in range(len(kinds)):
            frames = G.frames_of(pcm[:, j].reshape(-1).astype(np.float64) / 32768.0, *win_hop(opr))[-T:]
            if len(frames):
                r32 = max(r32, err(restated(frames, opr)[0], feats[j, T - len(frames):]))
        return frozen(pcm), frozen(raw), frozen(feats), r32
    return shared(('stream', G.set_id(kw), chunk), make)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('chunk', [1024, 777], ids=['pairs1024', 'odd777'])         # dword-pair loads / sample-by-sample loads
@pytest.mark.parametrize('kw', G.LENGTHS, ids=G.set_id)
def test_streaming_kernel(kw, chunk, prec):
    pcm, want_raw, want_feats, r32 = stream_reference(kw, chunk)
    n = pcm.shape[1]
    w = weights_of(kw)
    eng, twin = engine(kw, w, n, prec), engine(kw, w, n, prec)
    perm = np.random.default_rng(5).permutation(n)
    worst = 0.0
    for u in range(N_UPDATES):
        raw = eng.update(pcm[u])
        worst = max(worst, err(raw, want_raw[u]))
        if u == SUBSET_AT:                  # a permutation of all streams through the id indirection: the same bits, row by row
            sub = np.empty(n, np.float32)
            sub[perm] = twin.update_subset(perm, pcm[u][perm])
        else:
            sub = twin.update(pcm[u])
        assert np.array_equal(sub, raw), u
    feats = eng.get_vectors()
    assert feats.shape == want_feats.shape
    assert np.array_equal(twin.get_vectors(), feats)
    assert all(np.array_equal(x, y) for x, y in zip(eng.stream_state(), twin.stream_state()))
    eng.close(); twin.close()
    hold(kw, prec, 'stream%d' % chunk, 'probabilities', worst, None, GUARD_RAW, TOL_RAW)
    hold(kw, prec, 'stream%d' % chunk, 'ring rows', err(feats, want_feats), r32, TOL_FEAT32, CAP_FEAT_F32)


# ---- 3. clips kernel -----------------------------------------------------------------------------------------------------
def clip_lengths(opr):
    """clips of 0, 1, 1, 2, n_features - 1 and n_features frames, and one longer than max_samples (cropped to its tail)"""
    W, H, T = opr.window_samples, opr.hop_samples, opr.n_features
    return [W - 1, W, W + H - 1, W + H, W + (T - 1) * H - 1, W + (T - 1) * H, opr.max_samples + 1234]


def make_clips(lengths, first_seed=0):
    return [synth.stream_pcm(first_seed + i, int(n)).astype(np.float64) / 32768.0 for i, n in enumerate(lengths)]


def padded(rows, T):
    """vectorization.py:62-84: left zero pad / tail crop to T rows"""
    if len(rows) < T:
        rows = np.concatenate([np.zeros((T - len(rows), rows.shape[1])), rows])
    return rows[-T:]


def clips_reference(kw):
    def make():
        opr = ol.Params(**kw)
        clips = make_clips(clip_lengths(opr), 300)
        T = opr.n_features
        want = np.stack([ol.vectorize(c, opr) for c in clips])
        want_mels = np.stack([padded(sr.mel_spec(c[-opr.max_samples:], opr.sample_rate, win_hop(opr), opr.n_fft, opr.n_filt), T) for c in clips])
        r32 = r32_mels = 0.0
        for c, clip in enumerate(clips):
            frames = G.frames_of(clip[-opr.max_samples:], *win_hop(opr))[-T:]
            if len(frames):
                m32, l32 = restated(frames, opr)
                r32, r32_mels = max(r32, err(m32, want[c, T - len(frames):])), max(r32_mels, err(l32, want_mels[c, T - len(frames):]))
        return [frozen(c) for c in clips], frozen(want), frozen(want_mels), r32, r32_mels
    return shared(('clips', G.set_id(kw)), make)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('kw', G.LENGTHS, ids=G.set_id)
def test_clips_kernel(kw, prec):
    clips, want, want_mels, r32, r32_mels = clips_reference(kw)
    opr = ol.Params(**kw)
    eng = engine(kw, weights_of(kw), prec=prec)
    got = eng.vectorize_clips(clips, opr.max_samples)
    got_mels = eng.vectorize_clips(clips, opr.max_samples, mels=True)
    assert got.shape == want.shape == (7, opr.n_features, kw['n_mfcc']) and got_mels.shape == want_mels.shape
    assert np.all(got[0] == 0) and np.all(got[1][:-1] == 0) and np.any(got[1][-1] != 0)         # no frame: all pad rows; one frame: the last row
    assert np.all(got[4][0] == 0) and np.any(got[5][0] != 0)                                      # n_features - 1 frames: one pad row; n_features: none
    # a frame's bits do not depend on the entry point: the rows vectorize_raw returns for the same samples
    for c, clip in enumerate(clips):
        raw, raw_mels = eng.vectorize_raw(clip[-opr.max_samples:]), eng.vectorize_mels(clip[-opr.max_samples:])
        cast = (lambda a: a) if prec == 'f64' else (lambda a: a.astype(np.float32))
        assert np.array_equal(cast(padded(raw, opr.n_features)), cast(got[c])), c
        assert np.array_equal(cast(padded(raw_mels, opr.n_features)), cast(got_mels[c])), c
    eng.close()
    hold(kw, prec, 'clips', 'features', err(got, want), r32, TOL_MFCC, CAP_FEAT_F32)
    hold(kw, prec, 'clips', 'mels', err(got_mels, want_mels), r32_mels, TOL_MFCC, CAP_FEAT_F32)


# ---- 4. recordings kernel ------------------------------------------------------------------------------------------------
HOP_FRAMES = 3


def recs_reference(kw):
    """three recordings of n_features + 1, + 11 and + 30 frames (1, 4 and 10 windows), with odd samples left over: the oracle's
    strided windows through the network, and the same windows of float32-restated rows through it"""
    def make():
        opr = ol.Params(**kw)
        W, H, T = opr.window_samples, opr.hop_samples, opr.n_features
        w = weights_of(kw)
        recs = make_clips([W + T * H + 7, W + (T + 10) * H + H - 1, W + (T + 29) * H + 1], 500)
        want, r32 = [], 0.0
        for r in recs:
            mf = sr.mfcc_spec(r, opr.sample_rate, (W, H), opr.n_fft, opr.n_filt, opr.n_mfcc)
            starts = range(T, len(mf), HOP_FRAMES)
            want.append(frozen(keras_gru.predict(np.stack([mf[i - T:i] for i in starts]), w)))
            m32 = restated(G.frames_of(r, W, H), opr)[0]
            r32 = max(r32, err(keras_gru.predict(np.stack([m32[i - T:i] for i in starts]), w), want[-1]))
        return [frozen(r) for r in recs], want, r32
    return shared(('recs', G.set_id(kw)), make)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('kw', G.LENGTHS, ids=G.set_id)
def test_recordings_kernel(kw, prec):
    recs, want, r32 = recs_reference(kw)
    eng = engine(kw, weights_of(kw), prec=prec)
    got = eng.evaluate_clips(recs, HOP_FRAMES)
    assert [g.shape for g in got] == [w.shape for w in want] == [(1, 1), (4, 1), (10, 1)]
    for g, r in zip(got, recs):             # the same windows through the offline kernel
        assert np.array_equal(g, eng.evaluate(r, HOP_FRAMES))
    eng.close()
    worst = max(err(g, w) for g, w in zip(got, want))
    hold(kw, prec, 'recs', 'probabilities', worst, None, GUARD_RAW, TOL_RAW)
    print('GENLEN-NOTE | %s | %s | recs | probabilities of float32-restated rows | %.3g |' % (G.set_id(kw), prec, r32))
