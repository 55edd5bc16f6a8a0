"""GPU: many long recordings evaluated and measured in one call (pe_evaluate_clips / pe_simulate_scores / pe_simulate_clips)
-- precise-simulate (scripts/simulate.py:106-129) and compute_nww_annoyances (annoyance_estimator.py:56-73) without the
per-recording loop.  The predictions are gated by bit-identity to ``evaluate`` per recording; the metrics by an oracle that
lives here: the project's own ``runner.TriggerDetector`` (pinned by tests/golden/precise_runner.npz) fed ``float(p)``,
``math.fsum``, and ``(p.astype(float64)[:, None] > thr).sum(0)``.  That oracle is held in turn to the script itself:
tests/golden/simulate.npz is what the reference's own ``SimulateScript.run`` computed and printed (tools/make_script_fixtures.py);
test_simulate_host.py asks ``host_metric`` for its counts and sums and ``simulate.Metric`` for its report, and that a window stride
of ``hop_frames +- 1`` does NOT give its predictions; the last test here reads the same file on the device."""
import math

import numpy as np
import pytest

from mycroft_precise_amd import synth
from mycroft_precise_amd import params as P
from mycroft_precise_amd.runner import TriggerDetector
from mycroft_precise_amd.simulate import default_thresholds
from oracle import listener as ol, keras_gru

pytestmark = pytest.mark.gpu

TOL_RAW = 1e-4
# stock params: window 1600, hop 800, T = 29: f frames need 1600 + 800 (f - 1) samples.  24000: 29 frames, no window;
# 24800: 30 frames, one window whatever the hop; 28800: 35 frames, two windows at hop_frames = 5
EDGE_LENGTHS = [0, 1, 1599, 24000, 24800, 25599, 28000, 28800, 28801]
T = 29


def frames_of(n):
    return 1 + (n - 1600) // 800 if n >= 1600 else 0


def windows_of(n, hop_frames):
    return len(range(T, frames_of(n), hop_frames))


def make_recordings(lengths, first_seed=0):
    return [synth.stream_pcm(first_seed + i, int(n)).astype(np.float64) / 32768.0 for i, n in enumerate(lengths)]


@pytest.fixture(scope='module')
def lengths():
    rng = np.random.default_rng(20241)
    out = EDGE_LENGTHS + [int(v) for v in rng.integers(1, 200001, 40)]
    # the set as the stock tools see it (chunk_size 4096: hop_frames 5): recordings without a window, with exactly one, and
    # enough windows for several words of 64 per recording and several tiles of 16 per launch
    counts = [windows_of(n, 5) for n in out]
    assert 0 in counts and 1 in counts and counts[7] == 2 and sum(counts) >= 200
    return out


@pytest.fixture(scope='module')
def recordings(lengths):
    recs = make_recordings(lengths)
    for r in recs:
        r.setflags(write=False)
    return recs


@pytest.fixture(scope='module')
def oracle_scores(recordings, stock_weights):
    """the oracle's predictions of the standard set at hop_frames = 5 (computed once, shared, never written to)"""
    out = []
    for a in recordings:
        feats = ol.vectorize_raw(a, ol.Params()) if len(a) >= 1600 else np.zeros((0, 13))
        x = [feats[i - T:i] for i in range(T, len(feats), 5)]
        p = keras_gru.predict(np.array(x), stock_weights).reshape(-1) if x else np.zeros(0)
        p.setflags(write=False)
        out.append(p)
    return out


def engine(weights, n_streams=1, params=None, **kw):
    from mycroft_precise_amd._lib import HipEngine
    return HipEngine(params or P.pr, weights, n_streams=n_streams, **kw)


def offsets_of(recs):
    return np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)


def assert_equal_lists(got, want, what=''):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype == np.float32, (what, r, g.shape, w.shape)
        assert np.array_equal(g, w), (what, r)


# ---- the metrics oracle ----------------------------------------------------------------------------------------------
def host_metric(p, chunk_threshold, sensitivity, trigger_level, chunk_size):
    """(n_windows, activated_chunks, activations, fsum) of one recording's float32 predictions"""
    p = np.asarray(p, dtype=np.float32).reshape(-1)
    det = TriggerDetector(chunk_size, sensitivity, trigger_level)
    acts = sum(bool(det.update(float(x))) for x in p)
    return len(p), int((p.astype(np.float64) > chunk_threshold).sum()), acts, math.fsum(float(x) for x in p)


def host_buckets(per_recording, thr):
    p = np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1) for x in per_recording]) if per_recording else np.zeros(0, np.float32)
    return (p.astype(np.float64)[:, None] > np.asarray(thr, dtype=np.float64)).sum(0)


def assert_metrics(rows, per_recording, chunk_threshold, sensitivity, trigger_level, chunk_size, what=''):
    """rows: SIM_METRIC [n_rec] of one model"""
    assert rows.shape == (len(per_recording),)
    for r, p in enumerate(per_recording):
        n, chunks, acts, fsum = host_metric(p, chunk_threshold, sensitivity, trigger_level, chunk_size)
        row = rows[r]
        assert (int(row['n_windows']), int(row['activated_chunks']), int(row['activations'])) == (n, chunks, acts), (what, r)
        # the float64 summation bound: n - 1 additions in any order, each within 2^-53 relative of a partial sum <= the total
        assert abs(float(row['activation_sum']) - fsum) <= n * 2.0 ** -53 * fsum, (what, r, float(row['activation_sum']), fsum)


# ---- 1. bit-identity to evaluate ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('hop_frames', [1, 2, 5, 29, 40])
@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_evaluate_clips_equals_evaluate_bitwise(stock_weights, lengths, recordings, prec, hop_frames):
    eng = engine(stock_weights, mfcc_precision=prec)
    counts = [windows_of(n, hop_frames) for n in lengths]
    assert 0 in counts and 1 in counts
    woff = eng.evaluate_clips_layout(offsets_of(recordings), hop_frames)
    assert woff.dtype == np.int64 and woff.tolist() == [0] + np.cumsum(counts).tolist()
    recs32 = [r.astype(np.float32) for r in recordings]                   # (int16 / 32768: exact in float32)
    assert all(np.array_equal(a.astype(np.float64), b) for a, b in zip(recs32, recordings))
    for form in (0, 1, 2):
        eng.set_gru_tiling(form)
        assert eng.gru_tiling() == form
        want = [eng.evaluate(r, hop_frames) for r in recordings]
        assert [len(w) for w in want] == counts
        for sent in (recordings, recs32):
            assert_equal_lists(eng.evaluate_clips(sent, hop_frames), want, (form, sent is recs32))
    eng.close()


# ---- 2. other engine kinds ---------------------------------------------------------------------------------------------
SUB = EDGE_LENGTHS + [31337, 90001, 47999, 123456, 64000, 199999]


def check_against_evaluate(eng, recs, hops=(5, 3)):
    for hop_frames in hops:
        want = [eng.evaluate(r, hop_frames) for r in recs]
        assert sum(w.shape[-2] for w in want) > 60
        assert_equal_lists(eng.evaluate_clips(recs, hop_frames), want, hop_frames)
        assert_equal_lists(eng.evaluate_clips([r.astype(np.float32) for r in recs], hop_frames), want, hop_frames)


def test_speechpy_front_end(stock_weights):
    hpr = P.pr.copy()
    hpr.__dict__['vectorizer'] = P.Vectorizer.speechpy_mfccs
    eng = engine(stock_weights, params=hpr)
    recs = make_recordings(SUB, 100)
    # one frame fewer (vectorization.py:46-50 with the speechpy entry): 24800 samples are 29 frames, no window
    assert len(eng.evaluate(recs[4], 5)) == 0 and len(eng.evaluate(recs[5], 5)) == 0 and len(eng.evaluate(recs[7], 5)) == 1
    check_against_evaluate(eng, recs)
    eng.close()


@pytest.mark.parametrize('prec', ['f64', 'f32'])
def test_general_front_end(prec):
    import warnings
    kw = dict(n_fft=1024, n_filt=40, n_mfcc=20)
    hpr = P.pr.copy()
    hpr.__dict__.update(kw)
    w = synth.make_weights(n_in=20, units=(8,), seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        eng = engine(w, params=hpr, mfcc_precision=prec)
    check_against_evaluate(eng, make_recordings(SUB, 200))
    eng.close()


def test_use_delta():
    w = synth.make_weights(n_in=26, units=(20,), seed=77)
    hpr = P.pr.copy()
    hpr.__dict__['use_delta'] = True
    eng = engine(w, params=hpr)
    recs = make_recordings(SUB, 300)
    recs[9] = synth.stream_pcm(9, 40000, 'square').astype(np.float64) / 32768.0     # loud rows right in front of the next recording
    for tiling in (0, 1):
        eng.set_gru_tiling(tiling)
        check_against_evaluate(eng, recs)
    eng.close()


@pytest.mark.parametrize('ring', ['f32', 'bf16'])
def test_bf16_network(stock_weights, ring):
    eng = engine(stock_weights, gru_precision='bf16', ring_precision=ring)
    recs = make_recordings(SUB, 400)
    for tiling in (-1, 0):
        eng.set_gru_tiling(tiling)
        check_against_evaluate(eng, recs, hops=(5,))
    eng.close()


def test_three_models_share_the_front_end(stock_weights):
    recs = make_recordings(SUB, 500)
    ws = [stock_weights, synth.make_weights(seed=5), synth.make_weights(seed=6)]
    multi = engine(ws)
    got = multi.evaluate_clips(recs, 5)
    want = [multi.evaluate(r, 5) for r in recs]
    assert got[-1].shape == (3, windows_of(199999, 5), 1)
    assert_equal_lists(got, want)
    multi.set_clip_pass_bytes(700000)                # K models across passes: every model's block in its place
    assert_equal_lists(multi.evaluate_clips(recs, 5), want)
    metrics, buckets, scores = multi.simulate_clips(recs, 5, 0.5, 0.5, 0, 4096, [0.3, 0.5, 0.7], return_scores=True)
    assert metrics.shape == (3, len(recs)) and buckets.shape == (3, 3)
    assert_equal_lists(scores, want)
    for m, w in enumerate(ws):
        single = engine(w)
        assert_equal_lists(single.evaluate_clips(recs, 5), [g[m] for g in got], m)
        single.close()
        assert_metrics(metrics[m], [g[m] for g in got], 0.5, 0.5, 0, 4096, m)
        assert np.array_equal(buckets[m], host_buckets([g[m] for g in got], [0.3, 0.5, 0.7]))
    assert len({buckets[m].tobytes() for m in range(3)}) == 3          # three different models: three different rows
    multi.close()


@pytest.mark.parametrize('tiling', [0, 2])
def test_wide_network(tiling):
    w = synth.make_weights(units=(64, 64), seed=564)
    eng = engine(w)
    eng.set_gru_tiling(tiling)
    check_against_evaluate(eng, make_recordings(SUB, 600), hops=(5,))
    eng.close()


# ---- 3. passes ---------------------------------------------------------------------------------------------------------
def test_pass_size_does_not_change_a_bit(stock_weights, recordings):
    eng = engine(stock_weights)
    thr = default_thresholds()
    args = (5, 0.45, 0.55, 0, 4096, thr)
    base_m, base_b, base_s = eng.simulate_clips(recordings, *args, return_scores=True)     # the default target: one pass
    assert base_m['activated_chunks'].sum() > 0 and base_b[0] == base_m['n_windows'].sum() >= 200
    total_bytes = 8 * sum(len(r) for r in recordings)
    for target in (1, total_bytes // 5, 256 << 20):          # one recording per pass; a handful of passes; the default
        eng.set_clip_pass_bytes(target)
        for sent in (recordings, [r.astype(np.float32) for r in recordings]):
            m, b, s = eng.simulate_clips(sent, *args, return_scores=True)
            assert_equal_lists(s, base_s, target)
            assert_equal_lists(eng.evaluate_clips(sent, 5), base_s, target)
            assert m.tobytes() == base_m.tobytes(), target             # (activation_sum included, bit for bit)
            assert np.array_equal(b, base_b), target
    eng.close()


# ---- 4. the metrics kernels on crafted predictions ----------------------------------------------------------------------
SEQ_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 1000]
DENSITIES = [0.0, 0.02, 0.3, 0.9, 1.0]
REPEATED = [0.0, 0.1, 0.25, 0.25, 0.5, 0.5, 0.5, 0.75, 1.0, 1.0]     # (0.25, 0.5, 0.75, 0, 1: exact in float32 -- met below)


def crafted(seed, thr):
    """one sequence per (length, density) and the docstring pattern of the reference's TriggerDetector, `...!!!..!!...`,
    several times over, in one fixed order whatever the seed; hot means > 0.5.  0.0, 1.0, 0.25, 0.5, 0.75 (each equal to a
    threshold of REPEATED) and the float32 neighbours of some thresholds of `thr` are sprinkled in."""
    rng = np.random.default_rng(seed)
    special = np.concatenate([[0.0, 1.0, 0.5, 0.25, 0.75], np.asarray(thr, dtype=np.float64).astype(np.float32)[::37]]).astype(np.float32)
    seqs = []
    for n in SEQ_LENGTHS:
        for d in DENSITIES:
            hot = rng.random(n) < d
            p = np.where(hot, rng.uniform(0.5, 1.0, n), rng.uniform(0.0, 0.5, n)).astype(np.float32)
            p[hot & (p <= 0.5)] = np.float32(0.75)            # (a rounding to exactly 0.5 would not be hot)
            k = rng.random(n) < 0.1
            p[k] = rng.choice(special, int(k.sum()))
            seqs.append(p)
    pattern = np.array([0.9 if c == '!' else 0.1 for c in '...!!!..!!...' * 11], dtype=np.float32)
    seqs.append(pattern)
    order = np.random.default_rng(99).permutation(len(seqs))
    return [seqs[i] for i in order]


def crosses_a_word_in_rearm(p, sensitivity, trigger_level, chunk_size):
    """does a rearm period (activation < 0 after a fire) reach across a multiple of 64 windows?"""
    det = TriggerDetector(chunk_size, sensitivity, trigger_level)
    for i, x in enumerate(p):
        if i and i % 64 == 0 and det.activation < 0:
            return True
        det.update(float(x))
    return False


@pytest.mark.parametrize('chunk_size', [1024, 2048, 4096, 20000])
@pytest.mark.parametrize('trigger_level', [0, 3])
def test_simulate_scores_on_crafted_predictions(stock_weights, trigger_level, chunk_size):
    assert -(8 * 2048) // 20000 == -1 and -(8 * 2048) // 1024 == -16
    eng = engine([stock_weights, synth.make_weights(seed=5)])           # K = 2; no network runs
    seen_acts, seen_cross = 0, False
    for thr in (default_thresholds(), np.array(REPEATED)):
        a, b = crafted(1, thr), crafted(2, thr)              # the same lengths for both models, a different sequence for each
        assert [len(x) for x in a] == [len(x) for x in b]
        empties = [i for i, s in enumerate(a) if len(s) == 0]
        assert empties and 0 < empties[0] and empties[-1] < len(a) - 1          # recordings before and after an empty one
        scores = [np.stack([x, y]) for x, y in zip(a, b)]
        assert any(not np.array_equal(x, y) for x, y in zip(a, b))
        metrics, buckets = eng.simulate_scores(scores, 0.3, 0.5, trigger_level, chunk_size, thr)
        assert metrics.shape == (2, len(a)) and buckets.shape == (2, len(thr)) and buckets.dtype == np.int64
        for m, seqs in enumerate((a, b)):
            assert_metrics(metrics[m], seqs, 0.3, 0.5, trigger_level, chunk_size, (m, len(thr)))
            assert np.array_equal(buckets[m], host_buckets(seqs, thr)), (m, len(thr))
            seen_acts += int(metrics[m]['activations'].sum())
            seen_cross = seen_cross or any(crosses_a_word_in_rearm(s, 0.5, trigger_level, chunk_size) for s in seqs)
            allp = np.concatenate(seqs).astype(np.float64)
            assert (allp == 0).any() and (allp == 1).any()
            if len(thr) == len(REPEATED):
                assert all((allp == v).any() for v in REPEATED if v != 0.1)
        # the same bits again: nothing of the result depends on the run
        again_m, again_b = eng.simulate_scores(scores, 0.3, 0.5, trigger_level, chunk_size, thr)
        assert again_m.tobytes() == metrics.tobytes() and np.array_equal(again_b, buckets)
        # no thresholds: no buckets, the same metrics
        none_m, none_b = eng.simulate_scores(scores, 0.3, 0.5, trigger_level, chunk_size)
        assert none_m.tobytes() == metrics.tobytes() and none_b.shape == (2, 0)
    assert seen_acts > 0 and seen_cross
    eng.close()


def test_simulate_scores_one_model_and_other_settings(stock_weights):
    """a one-model engine (no leading axis), a sensitivity other than 0.5 and a negative trigger level"""
    eng = engine(stock_weights)
    seqs = crafted(7, REPEATED)
    for sens, chunk_thr, level in ((0.2, 0.8, 3), (0.9, 0.0, 1), (0.5, 1.0, -1)):
        metrics, buckets = eng.simulate_scores([s.reshape(-1, 1) for s in seqs], chunk_thr, sens, level, 2048, REPEATED)
        assert metrics.shape == (len(seqs),) and buckets.shape == (len(REPEATED),)
        assert_metrics(metrics, seqs, chunk_thr, sens, level, 2048, sens)
        assert np.array_equal(buckets, host_buckets(seqs, REPEATED))
    eng.close()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------
def test_simulate_clips_end_to_end(stock_weights, recordings, oracle_scores):
    eng = engine(stock_weights)
    scores = eng.evaluate_clips(recordings, 5)
    flat = np.concatenate(scores).reshape(-1)
    n = flat.size
    assert n == sum(len(p) for p in oracle_scores) >= 200 and len(np.unique(flat)) >= 8
    assert np.abs(flat.astype(np.float64) - np.concatenate(oracle_scores)).max() <= TOL_RAW
    thr = np.quantile(flat.astype(np.float64), [0.1, 0.5, 0.9])
    for q in thr:
        want_m, want_b = eng.simulate_scores(scores, q, 1.0 - q, 0, 4096, thr)
        assert 0 < want_m['activated_chunks'].sum() < n
        assert_metrics(want_m, scores, q, 1.0 - q, 0, 4096, q)
        assert np.array_equal(want_b, host_buckets(scores, thr)) and 0 < want_b[2] < want_b[1] < want_b[0] < n
        m, b, s = eng.simulate_clips(recordings, 5, q, 1.0 - q, 0, 4096, thr, return_scores=True)
        assert_equal_lists(s, scores)
        assert m.tobytes() == want_m.tobytes() and np.array_equal(b, want_b)
        m, b, s = eng.simulate_clips(recordings, 5, q, 1.0 - q, 0, 4096, thr)          # out = NULL
        assert s is None and m.tobytes() == want_m.tobytes() and np.array_equal(b, want_b)
    eng.close()


def test_runner_and_report(stock_weights, recordings):
    from mycroft_precise_amd.network_runner import HipRunner
    from mycroft_precise_amd import simulate as S
    runner = HipRunner(weights=stock_weights)
    sub = list(recordings[:16])
    want = [runner.evaluate(r) for r in sub]
    assert_equal_lists(runner.evaluate_clips(sub), want)
    metrics, total = S.simulate_recordings(runner, sub, threshold=0.45)
    kept = [i for i, r in enumerate(sub) if len(r)]
    assert len(metrics) == len(kept) == len(sub) - 1                       # the empty recording is skipped (simulate.py:110)
    check = S.Metric(4096)
    for m, i in zip(metrics, kept):
        n, chunks, acts, fsum = host_metric(want[i], 0.45, 0.45, 0, 4096)
        assert (m.seconds, m.activated_chunks, m.activations) == (len(sub[i]) / 16000, chunks, acts)
        assert abs(m.activation_sum - fsum) <= n * 2.0 ** -53 * fsum
        check.add(m)
    assert check == total and total.info_string('Total').startswith('=== Total ===\nHours: ')
    thr = S.default_thresholds()
    b = S.nww_buckets(runner, sub)
    assert b.dtype == np.float64 and np.array_equal(b, host_buckets(want, thr))
    assert np.array_equal(S.nww_buckets(runner, sub, thresholds=[0.2, 0.6]), host_buckets(want, [0.2, 0.6]))
    with pytest.raises(ValueError):
        runner.evaluate_clips(sub, chunk_size=799)


# ---- 6. validation -----------------------------------------------------------------------------------------------------
def test_validation_leaves_the_outputs_untouched(stock_weights, recordings):
    from mycroft_precise_amd._lib import SIM_METRIC
    eng = engine(stock_weights)
    lib, h = eng._lib, eng._h
    recs = list(recordings[4:8])                          # 1 + 1 + 1 + 2 windows at hop_frames = 5
    audio = np.concatenate(recs)
    good = offsets_of(recs)
    nan = float('nan')
    woff = np.full(5, -7, dtype=np.int64)
    out = np.full(8, 7.25, dtype=np.float32)
    metrics = np.zeros(4, dtype=SIM_METRIC)
    metrics['n_windows'] = -7
    buckets = np.full(3, -7, dtype=np.int64)
    thr = np.array([0.2, 0.5, 0.5])
    raw = np.linspace(0, 1, 5).astype(np.float32)
    good_w = np.array([0, 1, 2, 3, 5], dtype=np.int64)

    def p(a):
        return None if a is None else a.ctypes.data

    def layout(off=good, n=4, hop=5, dst=woff):
        return lib.pe_evaluate_clips_layout(h, p(off), n, hop, p(dst))

    def evaluate(a=audio, fmt=0, off=good, n=4, hop=5, dst=out, cap=8):
        return lib.pe_evaluate_clips(h, p(a), fmt, p(off), n, hop, p(dst), cap)

    def sim_clips(a=audio, fmt=0, off=good, n=4, hop=5, ct=0.5, sens=0.5, level=0, chunk=4096, t=thr, nt=3, m=metrics, b=buckets, dst=out, cap=8):
        return lib.pe_simulate_clips(h, p(a), fmt, p(off), n, hop, ct, sens, level, chunk, p(t), nt, p(m), p(b), p(dst), cap)

    def sim_scores(r=raw, stride=5, w=good_w, n=4, ct=0.5, sens=0.5, level=0, chunk=4096, t=thr, nt=3, m=metrics, b=buckets):
        return lib.pe_simulate_scores(h, p(r), stride, p(w), n, ct, sens, level, chunk, p(t), nt, p(m), p(b))

    decreasing = np.array([0, good[2], good[1], good[3], good[4]], dtype=np.int64)
    late = good + 1
    bad = [
        (layout, dict(off=None), 'null'), (layout, dict(dst=None), 'null'), (layout, dict(n=-1), 'n_rec'),
        (layout, dict(off=decreasing), 'recording 1'), (layout, dict(off=late), r'offsets\[0\]'), (layout, dict(hop=0), 'hop_frames'),
        (evaluate, dict(a=None), 'null'), (evaluate, dict(off=None), 'null'), (evaluate, dict(dst=None), 'null'),
        (evaluate, dict(n=-1), 'n_rec'), (evaluate, dict(fmt=2), 'sample_format'), (evaluate, dict(off=decreasing), 'recording 1'),
        (evaluate, dict(off=late), r'offsets\[0\]'), (evaluate, dict(hop=0), 'hop_frames'), (evaluate, dict(hop=-3), 'hop_frames'),
        (evaluate, dict(cap=4), 'need 5'),
        (sim_clips, dict(a=None), 'null'), (sim_clips, dict(off=None), 'null'), (sim_clips, dict(m=None), 'null'),
        (sim_clips, dict(b=None), 'null'), (sim_clips, dict(t=None), 'null'), (sim_clips, dict(n=-1), 'n_rec'),
        (sim_clips, dict(off=decreasing), 'recording 1'), (sim_clips, dict(off=late), r'offsets\[0\]'), (sim_clips, dict(hop=0), 'hop_frames'),
        (sim_clips, dict(chunk=0), 'chunk_size'), (sim_clips, dict(sens=nan), 'sensitivity'), (sim_clips, dict(ct=nan), 'chunk_threshold'),
        (sim_clips, dict(cap=4), 'need 5'), (sim_clips, dict(t=np.array([0.5, 0.2, 0.7])), 'thresholds decrease at 1'),
        (sim_clips, dict(t=np.array([0.2, nan, 0.7])), r'thresholds\[1\]'), (sim_clips, dict(nt=-1), 'n_thresholds'),
        (sim_clips, dict(t=np.zeros(4097), nt=4097), 'n_thresholds'),
        (sim_scores, dict(r=None), 'null'), (sim_scores, dict(w=None), 'null'), (sim_scores, dict(m=None), 'null'),
        (sim_scores, dict(b=None), 'null'), (sim_scores, dict(n=-1), 'n_rec'), (sim_scores, dict(w=np.array([0, 2, 1, 3, 5], dtype=np.int64)), 'recording 1'),
        (sim_scores, dict(w=good_w + 1), r'window_offsets\[0\]'), (sim_scores, dict(stride=4), 'stride'), (sim_scores, dict(chunk=-1), 'chunk_size'),
        (sim_scores, dict(sens=nan), 'sensitivity'), (sim_scores, dict(ct=nan), 'chunk_threshold'),
        (sim_scores, dict(t=np.array([0.5, 0.2, 0.7])), 'thresholds decrease at 1'), (sim_scores, dict(t=np.array([nan, 0.2, 0.7])), r'thresholds\[0\]'),
        (sim_scores, dict(nt=4097), 'n_thresholds'),
    ]
    for fn, kw, match in bad:
        with pytest.raises(ValueError, match=match):
            eng._check(fn(**kw))
        assert np.all(woff == -7) and np.all(out == 7.25) and np.all(buckets == -7) and np.all(metrics['n_windows'] == -7), (fn.__name__, kw)
    # the Python surface raises the same way
    with pytest.raises(ValueError, match='hop_frames'):
        eng.evaluate_clips(recs, 0)
    with pytest.raises(ValueError, match='thresholds decrease'):
        eng.simulate_clips(recs, 5, 0.5, 0.5, 0, 4096, [0.5, 0.4])
    with pytest.raises(ValueError):
        eng.evaluate_clips([np.zeros((2, 3))], 5)
    # n_rec = 0: nothing happens, whatever else is handed over
    for rc in (layout(off=None, n=0), evaluate(a=None, off=None, n=0, dst=None), sim_clips(a=None, off=None, n=0, m=None, chunk=0),
               sim_scores(r=None, w=None, n=0, m=None, sens=nan)):
        assert rc == 0
    assert woff[0] == 0 and np.all(woff[1:] == -7) and np.all(out == 7.25) and np.all(buckets == -7) and np.all(metrics['n_windows'] == -7)
    assert eng.evaluate_clips([], 5) == [] and eng.simulate_clips([], 5, 0.5, 0.5, 0, 4096, thr)[0].shape == (0,)
    assert np.array_equal(eng.simulate_clips([], 5, 0.5, 0.5, 0, 4096, thr)[1], np.zeros(3, np.int64))
    # ... and the good calls do work on these arguments
    assert layout() == 0 and woff.tolist() == [0, 1, 2, 3, 5]
    assert evaluate() == 0 and sim_clips() == 0 and metrics['n_windows'].tolist() == [1, 1, 1, 2] and buckets[0] >= buckets[1] == buckets[2]
    assert np.all(out[5:] == 7.25) and np.array_equal(out[:5], np.concatenate(eng.evaluate_clips(recs, 5)).reshape(-1))
    assert sim_scores() == 0 and buckets.tolist() == [4, 2, 2] and metrics['activated_chunks'].tolist() == [0, 0, 0, 2]
    # only recordings without a window: metrics of zeros, no launch to wait for
    m, b, s = eng.simulate_clips(recordings[:4], 5, 0.5, 0.5, 0, 4096, thr, return_scores=True)
    assert m.tolist() == [(0, 0, 0, 0.0)] * 4 and b.tolist() == [0, 0, 0] and [x.shape for x in s] == [(0, 1)] * 4
    eng.close()


# ---- 7. statelessness --------------------------------------------------------------------------------------------------
def test_streams_are_untouched(stock_weights, recordings):
    n = 19
    pcm = synth.batch_pcm(n, 12, 1024)
    a, b = engine(stock_weights, n_streams=n), engine(stock_weights, n_streams=n)
    sub = list(recordings[:14])
    for u in range(12):
        ra = a.update(pcm[u])
        if u in (3, 7):
            state = a.stream_state()
            a.simulate_clips(sub, 5, 0.5, 0.5, 0, 4096, default_thresholds(), return_scores=True)
            a.evaluate_clips(sub, 2)
            a.simulate_scores([np.linspace(0, 1, 70, dtype=np.float32)], 0.5, 0.5, 3, 2048)
            assert all(np.array_equal(x, y) for x, y in zip(state, a.stream_state()))
        if u == 5:                                    # ... and behind an update still in flight
            a.wait()
        assert np.array_equal(ra, b.update(pcm[u])), u
    out = a.update_async(pcm[0])
    a.simulate_clips(sub[:6], 5, 0.5, 0.5, 0, 4096)             # drains the update in flight first
    assert np.array_equal(out, b.update(pcm[0]))
    assert np.array_equal(a.get_vectors(), b.get_vectors())
    a.close(); b.close()


# ---- the script itself: tests/golden/simulate.npz (tools/make_script_fixtures.py) ---------------------------------------------
@pytest.mark.parametrize('chunk_size', [1024, 2048, 4096])
def test_simulation_equals_the_scripts_own_report(stock_weights, chunk_size):
    """SimulateScript.run's own numbers and printed report over recordings with 0, 1, 63, 64 and 65 predictions: activated
    chunks and activations are equal, the sums follow assert_metrics' rule over the device's predictions, which lie within
    TOL_RAW of the script's, and the report is the script's wherever its last figure has room for that (string_safe)."""
    from conftest import golden
    from mycroft_precise_amd.network_runner import HipRunner
    from mycroft_precise_amd import simulate as S
    g = golden('simulate.npz')
    k = '_%d' % chunk_size
    off, woff, threshold = g['offsets'], g['window_offsets' + k], float(g['threshold'])
    audios = [g['pcm'][a:b].astype(np.float32) / np.float32(32767.0) for a, b in zip(off[:-1], off[1:])]
    want = [g['predictions' + k][a:b] for a, b in zip(woff[:-1], woff[1:])]
    flat = g['predictions' + k].astype(np.float64)
    assert min(np.abs(flat - threshold).min(), np.abs(flat - (1.0 - threshold)).min()) > TOL_RAW and threshold != 0.5
    runner = HipRunner(weights=stock_weights)
    scores = runner.evaluate_clips(audios, chunk_size)
    assert [len(s) for s in scores] == np.diff(woff).tolist()
    worst = float(np.abs(np.concatenate(scores).reshape(-1).astype(np.float64) - flat).max())
    print('chunk_size %d: %d predictions, worst |p - the script\'s| %.3g' % (chunk_size, flat.size, worst))
    assert worst <= TOL_RAW
    rows, _, _ = runner.simulate(audios, chunk_size, threshold)
    assert_metrics(rows, scores, threshold, threshold, 0, chunk_size)
    assert rows['activated_chunks'].tolist() == g['activated_chunks' + k].tolist()
    assert rows['activations'].tolist() == g['activations' + k].tolist() and max(rows['activations']) >= 2
    metrics, total = S.simulate_recordings(runner, audios, chunk_size=chunk_size, threshold=threshold)
    assert [m.seconds for m in metrics] == g['seconds' + k].tolist()
    assert [(m.activated_chunks, m.activations) for m in metrics] == list(zip(rows['activated_chunks'].tolist(), rows['activations'].tolist()))
    safe = g['string_safe' + k]
    for r, m in enumerate(metrics):
        lines, want_lines = m.info_string('rec%02d.wav' % r).splitlines(), str(g['file_strings' + k][r]).splitlines()
        assert lines[:4] == want_lines[:4] and (not safe[r] or lines == want_lines), (r, lines, want_lines)
    assert (total.seconds, total.activated_chunks, total.activations) == tuple(g['total' + k][:3])
    assert bool(g['total_string_safe' + k]) and total.info_string('Total') == str(g['total_string' + k])
    # the buckets at the script's two comparisons: `p > t` is its activated chunks
    thr = sorted([threshold, 1.0 - threshold])
    buckets = S.nww_buckets(runner, audios, thresholds=thr, chunk_size=chunk_size)
    assert np.array_equal(buckets, host_buckets(want, thr)) and buckets[thr.index(threshold)] == g['total' + k][1]
