"""GPU: models trained on Vectorizer.mels features, served end to end against tests/mels_reference.py.

Bars.  Raw outputs of a float32 network <= 1e-4 (the project's float32 parity bar), of a bf16 network <= 1e-2.  Rows of the
float64 front end: |got - want| <= 2^-24 |want| + 1e-9 -- half a float32 ulp from the store into the ring, plus the 1e-9 that
tests/test_gpu_parity.py holds vectorize_mels to.  Rows of the float32 front end: held as tests/test_general_lengths.py holds
its float32 rows -- its cap (2e-4) and GUARD_X (8) times the distance, measured here, of the float32 restatement of the same
frames (general_lengths_common.float32_restatement) from the float64 reference.

Saturation must not hide an error: every reference output used in an output comparison lies in (0.01, 0.99), asserted on the
reference before it is compared.  The seeds below (SEED, NETS) were chosen for that on the CPU over tone_noise and square
audio, partly filled windows included; where no seed of the first dozen did, the first-layer kernel is scaled by 0.5.  Silent
audio saturates these networks -- log-mel rows of silence are -36.04 -- so the offline test, which has a clip of zeros, takes
seed 1 with the first-layer kernel scaled by 0.1."""
import contextlib
import json
import warnings

import numpy as np
import pytest

import general_lengths_common as G
import mels_reference as M
import stats_reference as SR
from mycroft_precise_amd import model, synth
from mycroft_precise_amd import params as P

pytestmark = pytest.mark.gpu

TOL_RAW = 1e-4              # float32 network (README)
TOL_RAW_BF16 = 1e-2         # bf16 operands
CAP_FEAT_F32 = 2e-4         # tests/test_general_lengths.py
GUARD_X = 8.0               # tests/test_general_lengths.py
N_STREAMS = 20              # one full 16-stream tile and a partial one
N_UPDATES = 40

SHAPES = {                  # name -> front-end fields; which kernel serves it
    'default-512x20': dict(n_fft=512, n_filt=20),           # general front end (rows of more than 16 values), radix
    'stock-512x16': dict(n_fft=512, n_filt=16),             # the one-frame-per-wave kernel
    'boundary-512x32': dict(n_fft=512, n_filt=32),
    'radix-1024x24': dict(n_fft=1024, n_filt=24),
    'bluestein-400x20': dict(n_fft=400, n_filt=20),
}
# (make_weights seed, scale of the first-layer kernel) of the 20-unit network behind each shape: chosen on the CPU so that the
# reference's outputs stay inside (0.01, 0.99) over every update of every chunk mode
SEED = {'default-512x20': (3, 1.0), 'stock-512x16': (2, 1.0), 'boundary-512x32': (1, 0.5), 'radix-1024x24': (1, 1.0), 'bluestein-400x20': (6, 1.0)}
CHUNKS = ['pairs1024', 'odd1023', 'random']


def hip_params(kw):
    hpr = P.pr.copy()
    hpr.__dict__.update(vectorizer=P.Vectorizer.mels)
    hpr.__dict__.update(kw)
    return hpr


def engine(kw, weights, n_streams=1, prec='f64', **more):
    from mycroft_precise_amd._lib import HipEngine
    from mycroft_precise_amd import vectorization as V
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', V.UnverifiedFilterbank)
        return HipEngine(hip_params(kw), weights, n_streams=n_streams, mfcc_precision=prec, **more)


@contextlib.contextmanager
def global_params(**fields):
    """the process-global ``pr`` (what HipRunner, Listener and the .params overlay read) with ``fields``; put back afterwards"""
    saved = dict(P.pr.__dict__)
    P.pr.__dict__.update(fields)
    try:
        yield saved
    finally:
        P.pr.__dict__.clear()
        P.pr.__dict__.update(saved)


def frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


_CACHE = {}


def shared(key, make):
    """a reference is computed once, shared by the tests that need it, never written to"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def unsaturated(want):
    want = np.asarray(want, dtype=np.float64)
    assert want.size and 0.01 < want.min() and want.max() < 0.99, (float(want.min()), float(want.max()))
    return want


def err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) if np.size(want) else 0.0


def scaled_first_layer(w, s=0.1):
    k, rk, b = w['gru'][0]
    return dict(w, gru=[(k * np.float32(s), rk, b)] + list(w['gru'][1:]))


def chunk_lengths(mode):
    if mode == 'pairs1024':
        return [1024] * N_UPDATES
    if mode == 'odd1023':
        return [1023] * N_UPDATES
    return [int(v) for v in np.random.default_rng(17).integers(1, 2400, N_UPDATES)]


def stream_audio(lengths, n_streams=N_STREAMS):
    """int16 [n_streams, total]: tone_noise and square streams alternating.  The square waves have periods of 102 .. 138 samples:
    none divides a transform length used here -- a frame that holds whole periods has bins that are exactly zero, their
    log-mel values are logarithms of rounding noise, and the float32 restatement of the REFERENCE is then 6.5 away from its
    float64 form (n_fft 400, period 50: measured on the CPU)"""
    total = int(np.sum(lengths))
    return np.stack([synth.stream_pcm(s + 30, total, 'square') if s % 2 else synth.stream_pcm(s, total, 'tone_noise')
                     for s in range(n_streams)])


def stream_reference(name, mode, weights=None, use_delta=False, n_streams=N_STREAMS, key=None):
    """the reference listener over the same chunks: window rows and raw output after EVERY update, and how far the float32
    restatement of every frame of the audio is from the float64 rows"""
    kw = SHAPES[name]

    def make():
        pr = M.params(use_delta=use_delta, **kw)
        w = weights or scaled_first_layer(synth.make_weights(n_in=pr.feature_size, units=(20,), seed=SEED[name][0]), SEED[name][1])
        lengths = chunk_lengths(mode)
        pcm = stream_audio(lengths, n_streams)
        ref = M.BatchedMels(w, n_streams, pr)
        rows, raw, at = [], [], 0
        for n in lengths:
            raw.append(ref.update_raw(pcm[:, at:at + n]))
            rows.append(ref.mfccs.copy())
            at += n
        r32 = 0.0
        for j in range(n_streams):
            frames = G.frames_of(pcm[j].astype(np.float64) / 32768.0, pr.window_samples, pr.hop_samples)
            l32 = G.float32_restatement(frames, pr.n_fft, pr.n_filt, min(13, pr.n_filt), pr.sample_rate, with_mels=True)[1]
            r32 = max(r32, err(l32, M.mels_from_frames(frames, pr)))
        return w, lengths, frozen(pcm), frozen(np.stack(rows)), frozen(np.stack(raw)), r32
    return shared(key or ('stream', name, mode), make)


def hold_rows(label, prec, got, want, r32):
    """print the figures, then assert the bar of the precision"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want)
    worst = err(got, want)
    print('MELS | %s | %s | rows | %.3g | restated f32 %.3g |' % (label, prec, worst, r32))
    if prec == 'f64':
        assert np.all(np.abs(got - want) <= 2.0 ** -24 * np.abs(want) + 1e-9), (label, worst)
    else:
        assert worst <= CAP_FEAT_F32 and worst <= GUARD_X * r32, (label, worst, r32)


# ---- 1. streaming rows and outputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['f64', 'f32'])
@pytest.mark.parametrize('mode', CHUNKS)
@pytest.mark.parametrize('name', list(SHAPES))
def test_streaming_rows_and_outputs(name, mode, prec):
    from mycroft_precise_amd import vectorization as V
    from mycroft_precise_amd.network_runner import BatchedListener
    w, lengths, pcm, want_rows, want_raw, r32 = stream_reference(name, mode)
    unsaturated(want_raw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', V.UnverifiedFilterbank)
        eng = BatchedListener(w, N_STREAMS, mfcc_precision=prec, params=hip_params(SHAPES[name])).engine
    assert eng.row_width == SHAPES[name]['n_filt']
    rows, raw, at = [], [], 0
    for n in lengths:
        raw.append(eng.update(np.ascontiguousarray(pcm[:, at:at + n])))
        rows.append(eng.get_vectors())
        at += n
    eng.close()
    assert rows[0].shape == want_rows[0].shape
    worst = err(np.stack(raw), want_raw)
    print('MELS | %s %s | %s | outputs | %.3g |' % (name, mode, prec, worst))
    hold_rows('%s %s' % (name, mode), prec, np.stack(rows), want_rows, r32)
    assert worst <= TOL_RAW, worst


# ---- 2. one configuration, every path, the same bits -------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['default-512x20', 'stock-512x16'])
def test_every_path_gives_the_same_bits(name):
    w, lengths, pcm, want_rows, want_raw, _ = stream_reference(name, 'pairs1024')
    kw, n, U = SHAPES[name], N_STREAMS, 36
    chunks = [np.ascontiguousarray(pcm[:, u * 1024:(u + 1) * 1024]) for u in range(U)]
    base = engine(kw, w, n)
    outs = [base.update(c) for c in chunks]
    assert len({o.tobytes() for o in outs[30:]}) > 1
    assert err(np.stack(outs), want_raw[:U]) <= TOL_RAW
    # predict over the window as it stands == the last update's output
    rows = base.get_vectors()
    assert np.array_equal(base.predict(rows)[:, 0], outs[-1])
    # streaming rows == float32 of the offline rows of the same audio, from either offline entry point
    T = rows.shape[1]
    for j in (0, 1, n - 1):
        audio = pcm[j, :U * 1024].astype(np.float64) / 32768.0
        off = base.vectorize_mels(audio)
        assert off.shape[1] == kw['n_filt'] and np.array_equal(base.vectorize_raw(audio), off)
        assert np.array_equal(off[-T:].astype(np.float32), rows[j]), j
    base.close()
    # one launch per update and two (the stock kernel's mel rows always take two: recorded, not assumed to differ)
    two = engine(kw, w, n)
    two.set_fused(False)
    for u in range(U):
        assert np.array_equal(two.update(chunks[u]), outs[u]), u
    assert np.array_equal(two.get_vectors(), rows)
    two.close()
    many = engine(kw, w, n)
    many.reserve_updates(6, 1024)
    for u in range(0, U, 6):
        assert np.array_equal(many.update_many(np.stack(chunks[u:u + 6])), np.stack(outs[u:u + 6])), u
    many.close()
    sub = engine(kw, w, n)
    rng = np.random.default_rng(4)
    for u in range(U):
        ids = rng.permutation(n).astype(np.int32)
        assert np.array_equal(sub.update_subset(ids, chunks[u][ids]), outs[u][ids]), u
    assert np.array_equal(sub.get_vectors(), rows)
    # set_vectors(get_vectors) restarts the streams on the same window
    sub.set_vectors(rows)
    assert np.array_equal(sub.get_vectors(), rows)
    sub.close()


# ---- 3. offline: clips and recordings ----------------------------------------------------------------------------------------
def offline_reference(prm_kw):
    def make():
        pr = M.params(**prm_kw)
        W, H, T = pr.window_samples, pr.hop_samples, pr.n_features
        w = scaled_first_layer(synth.make_weights(n_in=pr.feature_size, units=(20,), seed=1))
        lengths = [W - 1, W, W + 5 * H + 3, W + (T - 1) * H - 1, pr.max_samples, pr.max_samples + 1234]
        clips = [synth.stream_pcm(300 + i, int(n), 'square' if i % 2 else 'tone_noise').astype(np.float64) / 32768.0
                 for i, n in enumerate(lengths)]
        clips.append(np.zeros(W + 3 * H))                                # 4 frames of silence behind the left zero pad
        feats = np.stack([M.vectorize(c, pr) for c in clips])
        scores = M.predict(feats, w, pr)
        recs = [synth.stream_pcm(500 + i, int(n), 'square' if i % 2 else 'tone_noise').astype(np.float64) / 32768.0
                for i, n in enumerate([W + T * H + 7, W + (T + 10) * H + H - 1, W - 3])]
        hop_frames = 4096 // H
        windows = []
        for r in recs:
            rows = M.vectorize_raw(r, pr)
            starts = range(T, len(rows), hop_frames)
            windows.append(frozen(M.predict(np.stack([rows[i - T:i] for i in starts]), w, pr)) if len(starts) else np.zeros(0, np.float32))
        return w, [frozen(c) for c in clips], frozen(feats), frozen(scores), [frozen(r) for r in recs], windows
    return shared(('offline',) + tuple(sorted(prm_kw.items())), make)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_offline_clips_and_recordings(prec):
    kw = SHAPES['default-512x20']
    with global_params(vectorizer=P.Vectorizer.mels, **kw):          # HipRunner reads the process-global parameters
        offline_case(kw, prec)


def offline_case(kw, prec):
    from mycroft_precise_amd.network_runner import HipRunner
    w, clips, want_feats, want_scores, recs, want_windows = offline_reference(kw)
    unsaturated(want_scores)
    unsaturated(np.concatenate(want_windows))
    pr = M.params(**kw)
    T = pr.n_features
    runner = HipRunner(weights=w, mfcc_precision=prec)
    eng = runner.engine
    # rows of every clip: pad rows are zeros, the silent clip's rows exactly float32(log(eps))
    feats = eng.vectorize_clips(clips, pr.max_samples)
    assert feats.shape == want_feats.shape == (7, T, 20)
    assert np.array_equal(eng.vectorize_clips(clips, pr.max_samples, mels=True), feats)
    assert np.all(feats[0] == 0) and np.all(feats[1][:-1] == 0) and np.any(feats[1][-1] != 0)
    assert np.all(feats[6][:T - 4] == 0)
    assert np.all(feats[6][T - 4:].astype(np.float32) == np.float32(np.log(np.finfo(float).eps)))
    if prec == 'f64':
        assert np.all(np.abs(feats - want_feats) <= 1e-9)
    # score_clips / predict_clips / test_clips
    scores = runner.predict_clips(clips)
    assert scores.shape == (7, 1)
    print('MELS | offline | %s | score_clips | %.3g |' % (prec, err(scores[:, 0], want_scores)))
    assert err(scores[:, 0], want_scores) <= TOL_RAW
    assert err(runner.predict(want_feats.astype(np.float32))[:, 0], want_scores) <= TOL_RAW
    targets = np.array([1, 0, 1, 0, 1, 0, 0], dtype=np.float32)
    thresholds = (0.3, 0.5, 0.7)
    sweep, tested = runner.test_clips(clips, targets, thresholds, return_scores=True)
    assert np.array_equal(tested, scores)
    counts = SR.counts(tested, targets, thresholds, 'f32')
    assert np.array_equal(sweep.false_pos, counts['neg_gt']) and np.array_equal(sweep.true_pos, counts['pos_gt'])
    assert sweep.n == 7 and sweep.n_pos == 3 and sweep.n_neg == 4
    # evaluate / evaluate_clips / simulate
    got = runner.evaluate_clips(recs, 4096)
    assert [g.shape[0] for g in got] == [len(x) for x in want_windows] and got[2].shape[0] == 0
    for g, x, r in zip(got, want_windows, recs):
        assert np.array_equal(g, runner.evaluate(r, 4096))
        assert err(g[:, 0], x) <= TOL_RAW
    metrics, buckets, sim_scores = runner.simulate(recs, 4096, 0.5, return_scores=True)
    for r in range(3):
        assert np.array_equal(sim_scores[r], got[r])
        assert metrics['n_windows'][r] == got[r].shape[0]
        assert metrics['activated_chunks'][r] == int((got[r].astype(np.float64) > 0.5).sum())
        assert abs(metrics['activation_sum'][r] - float(got[r].astype(np.float64).sum())) <= 1e-9
    eng.close()


# ---- 3b. the same three offline launches on the stock wave kernel (n_filt <= 16), both precisions ----------------------------
# (profiles/front_end_dispatch/README.md: the cells whole buffer / clip table / recording table x stock family x mel rows, which
#  nothing above reaches -- 'default-512x20' is served by the general front end)
STOCK_HOP_FRAMES = 3


def stock_offline_reference():
    def make():
        pr = M.params(**SHAPES['stock-512x16'])
        W, H, T = pr.window_samples, pr.hop_samples, pr.n_features
        w = scaled_first_layer(synth.make_weights(n_in=pr.feature_size, units=(20,), seed=2))
        # shorter than a window | a partly filled window | whole windows | longer than max_samples (cropped as a clip)
        a, b, c, d = [synth.stream_pcm(700 + i, int(n), 'square' if i % 2 else 'tone_noise').astype(np.float64) / 32768.0
                      for i, n in enumerate([W - 3, W + 5 * H + 3, W + (T + 2) * H + 3, W + (T + 6) * H + 1])]
        clips, recs = [a, b, d], [a, c, d]
        feats = np.stack([M.vectorize(x, pr) for x in clips])
        rows = [M.vectorize_raw(x, pr) for x in recs]
        windows = [M.predict(np.stack([r[i - T:i] for i in range(T, len(r), STOCK_HOP_FRAMES)]), w, pr) if len(r) > T else np.zeros(0, np.float32)
                   for r in rows]
        frames = np.concatenate([G.frames_of(x, W, H) for x in (b, c, d)])
        r32 = err(G.float32_restatement(frames, pr.n_fft, pr.n_filt, min(13, pr.n_filt), pr.sample_rate, with_mels=True)[1],
                  M.mels_from_frames(frames, pr))
        return (w, [frozen(x) for x in clips], frozen(feats), frozen(M.predict(feats, w, pr)), [frozen(x) for x in recs],
                frozen(rows[2]), [frozen(x) for x in windows], r32)
    return shared(('offline', 'stock-512x16'), make)


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_stock_kernel_offline_mel_rows(prec):
    w, clips, want_feats, want_scores, recs, want_rows, want_windows, r32 = stock_offline_reference()
    unsaturated(want_scores[1:])                    # (clip 0 is shorter than a window: every row a pad row)
    unsaturated(np.concatenate(want_windows))
    pr = M.params(**SHAPES['stock-512x16'])
    eng = engine(SHAPES['stock-512x16'], w, 1, prec)
    assert eng.row_width == 16

    def hold_offline(label, got, want):             # float64: the bar of offline_case; float32: the bar of hold_rows
        if prec == 'f64':
            print('MELS | stock offline %s | f64 | rows | %.3g |' % (label, err(got, want)))
            assert np.all(np.abs(got - want) <= 1e-9), (label, err(got, want))
        else:
            hold_rows('stock offline ' + label, prec, got, want, r32)
    # whole buffer
    off = eng.vectorize_mels(recs[2])
    assert off.shape == want_rows.shape and np.array_equal(eng.vectorize_raw(recs[2]), off)
    hold_offline('buffer', off, want_rows)
    # clip table
    feats = eng.vectorize_clips(clips, pr.max_samples)
    assert feats.shape == want_feats.shape == (3, pr.n_features, 16)
    assert np.all(feats[0] == 0) and np.all(feats[1][:-6] == 0) and np.all(feats[1][-6:] != 0)
    hold_offline('clips', feats, want_feats)
    scores = eng.score_clips(clips, pr.max_samples)
    print('MELS | stock offline | %s | score_clips | %.3g |' % (prec, err(scores[:, 0], want_scores)))
    assert scores.shape == (3, 1) and err(scores[:, 0], want_scores) <= TOL_RAW
    # recording table
    got = eng.evaluate_clips(recs, STOCK_HOP_FRAMES)
    assert [g.shape[0] for g in got] == [0, 1, 3] == [len(x) for x in want_windows]
    for g, x, r in zip(got, want_windows, recs):
        assert np.array_equal(g, eng.evaluate(r, STOCK_HOP_FRAMES))
        assert err(g[:, 0], x) <= TOL_RAW
    eng.close()


# ---- 4. networks -------------------------------------------------------------------------------------------------------------
NETS = {    # name -> (shape, units, use_delta, (make_weights seed, first-layer scale): unsaturated on the CPU, as SEED)
    '20u': ('default-512x20', (20,), False, (3, 1.0)),
    '64u-wide': ('default-512x20', (64,), False, (1, 1.0)),
    'stacked-40x24': ('default-512x20', (40, 24), False, (1, 0.5)),
    'delta-16filt': ('stock-512x16', (20,), True, (1, 1.0)),
}


@pytest.mark.parametrize('net', list(NETS))
def test_networks_behind_mel_rows(net):
    name, units, delta, (seed, scale) = NETS[net]
    n, kw = N_STREAMS, dict(SHAPES[name], use_delta=delta)
    n_in = SHAPES[name]['n_filt'] * (2 if delta else 1)
    w0 = scaled_first_layer(synth.make_weights(n_in=n_in, units=units, seed=seed), scale)
    w, lengths, pcm, want_rows, want_raw, _ = stream_reference(name, 'pairs1024', weights=w0, use_delta=delta, key=('net', net))
    unsaturated(want_raw)
    eng = engine(kw, w, n)
    assert eng.feature_size == n_in
    raw, at = [], 0
    for c in lengths:
        raw.append(eng.update(np.ascontiguousarray(pcm[:, at:at + c])))
        at += c
    rows = eng.get_vectors()
    eng.close()
    worst = err(np.stack(raw), want_raw)
    print('MELS | net %s | outputs | %.3g |' % (net, worst))
    assert np.all(np.abs(rows.astype(np.float64) - want_rows[-1]) <= 2.0 ** -24 * np.abs(want_rows[-1]) + 1e-9)
    assert worst <= TOL_RAW, worst


@pytest.mark.parametrize('ring', ['f32', 'bf16'])
def test_bf16_network_and_bf16_rows_behind_14_filters(ring):
    """n_filt 14 on the stock wave kernel, bf16 operands (the five-values form's limit: <= 14 inputs), float32 and bf16 rows"""
    SHAPES_14 = dict(n_fft=512, n_filt=14)
    pr = M.params(**SHAPES_14)
    w = synth.make_weights(n_in=14, units=(20,), seed=1)
    n, lengths = N_STREAMS, [1024] * N_UPDATES

    def make():
        pcm = stream_audio(lengths, n)
        ref = M.BatchedMels(w, n, pr)
        raw = [ref.update_raw(pcm[:, u * 1024:(u + 1) * 1024]) for u in range(N_UPDATES)]
        return frozen(pcm), frozen(np.stack(raw)), frozen(ref.mfccs.copy())
    pcm, want_raw, want_rows = shared(('bf16', 14), make)
    unsaturated(want_raw)
    eng = engine(SHAPES_14, w, n, gru_precision='bf16', ring_precision=ring)
    raw = np.stack([eng.update(np.ascontiguousarray(pcm[:, u * 1024:(u + 1) * 1024])) for u in range(N_UPDATES)])
    rows = eng.get_vectors().astype(np.float64)
    eng.close()
    print('MELS | bf16 net, %s rows | outputs | %.3g |' % (ring, err(raw, want_raw)))
    assert err(raw, want_raw) <= TOL_RAW_BF16
    if ring == 'f32':
        assert np.all(np.abs(rows - want_rows) <= 2.0 ** -24 * np.abs(want_rows) + 1e-9)
    else:       # a bf16 row: 8 significant bits, rounded to nearest where it is stored
        assert np.all(np.abs(rows - want_rows) <= (2.0 ** -8 + 2.0 ** -24) * np.abs(want_rows) + 1e-9)


def test_two_models_on_the_default_mels_shape():
    name, n = 'default-512x20', N_STREAMS
    w1, lengths, pcm, _, want1, _ = stream_reference(name, 'pairs1024')
    w3 = synth.make_weights(n_in=20, units=(20,), seed=6)
    _, _, _, _, want3, _ = stream_reference(name, 'pairs1024', weights=w3, key=('two-models', 6))
    unsaturated(want1), unsaturated(want3)
    eng = engine(SHAPES[name], [w1, w3], n)
    one = engine(SHAPES[name], w3, n)
    for u, c in enumerate(lengths):
        chunk = np.ascontiguousarray(pcm[:, u * c:(u + 1) * c])
        got = eng.update(chunk)
        assert got.shape == (2, n)
        assert err(got[0], want1[u]) <= TOL_RAW and err(got[1], want3[u]) <= TOL_RAW, u
        assert np.array_equal(got[1], one.update(chunk)), u
    eng.close(); one.close()


# ---- 5. the Python surface: a saved model with a .params file that says mels -------------------------------------------------
def test_listener_from_saved_model_matches_reference_listener(tmp_path):
    from mycroft_precise_amd.network_runner import Listener
    with global_params() as saved:                              # (inject_params overlays the process-global parameters)
        name = str(tmp_path / 'mels.npz')
        w = synth.make_weights(n_in=20, units=(20,), seed=3)
        model.save_weights(name, w)
        with open(name + '.params', 'w') as f:
            json.dump(dict(saved, vectorizer=P.Vectorizer.mels), f)
        lis = Listener(name, chunk_size=2048)
        assert lis.pr.vectorizer == P.Vectorizer.mels and lis.mfccs.shape == (lis.pr.n_features, 20)
        pr = M.params(threshold_config=tuple(map(tuple, saved['threshold_config'])), threshold_center=saved['threshold_center'])
        ref = M.MelsListener(w, pr, chunk_size=2048)
        pcm = synth.stream_pcm(2, 40 * 1024)
        chunks = [pcm[u * 1024:(u + 1) * 1024].tobytes() for u in range(40)]
        want, got = [], []
        for u, chunk in enumerate(chunks):                      # raw outputs and the window, chunk by chunk
            want.append(ref.update_raw32(chunk))
            got.append(lis.update_raw(chunk))
            rows = lis.mfccs
            assert rows.shape == ref.mfccs.shape
            assert np.all(np.abs(rows - ref.mfccs) <= 2.0 ** -24 * np.abs(ref.mfccs) + 1e-9), u
        unsaturated(want)
        assert err(got, np.array(want, dtype=np.float64)) <= TOL_RAW
        # decoder included: update() hands the network's float32 scalar to the ThresholdDecoder, as the reference does; the
        # reference's decoder over that same scalar is what it must return
        window = lis.mfccs
        lis.clear()
        for u, chunk in enumerate(chunks):
            assert lis.update(chunk) == ref.threshold_decoder.decode(np.float32(got[u])), u
        assert np.array_equal(lis.mfccs, window)
        # the window is settable, as the reference's plain attribute is
        lis.mfccs = ref.mfccs
        assert np.array_equal(lis.mfccs, ref.mfccs)
        assert np.array_equal(lis.runner.engine.get_vectors()[0], ref.mfccs.astype(np.float32))
        lis.runner.engine.close()


# ---- 6. mfccs engines are untouched by a mels engine in the same process ---------------------------------------------------
@pytest.mark.parametrize('kw', [dict(), dict(n_fft=1024, n_filt=40, n_mfcc=20)], ids=['stock', 'general'])
def test_mfcc_engine_unchanged_beside_a_mels_engine(kw):
    from mycroft_precise_amd._lib import HipEngine
    from oracle import listener as ol
    n, U = N_STREAMS, 34
    hpr = P.pr.copy()
    hpr.__dict__.update(kw)
    w = synth.make_weights(n_in=hpr.n_mfcc, units=(20,), seed=1)
    pcm = synth.batch_pcm(n, U)

    def run():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            eng = HipEngine(hpr, w, n_streams=n)
        out = np.stack([eng.update(pcm[u]) for u in range(U)])
        rows = eng.get_vectors()
        off = eng.vectorize_raw(pcm[:, 0].reshape(-1).astype(np.float64) / 32768.0)
        eng.close()
        return out, rows, off
    before = run()
    ref = ol.BatchedOracle(w, n, ol.Params(**kw))
    want = np.stack([ref.update_raw(pcm[u]) for u in range(U)])
    assert err(before[0], want) <= TOL_RAW
    mw = synth.make_weights(n_in=hpr.n_filt if hpr.n_filt <= 32 else 32, units=(20,), seed=1)
    mels = engine(dict(kw, n_filt=min(hpr.n_filt, 32)), mw, n)
    for u in range(4):
        mels.update(pcm[u])
    mels.vectorize_raw(pcm[:, 0].reshape(-1).astype(np.float64) / 32768.0)
    after = run()               # while the mels engine is alive
    mels.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
