"""GPU: trained models judged on the device (pe_stats_scores / pe_test_clips / pe_trainer_stats_models and the Python layers
over them) against the plain-numpy restatement (stats_reference.py, itself held to the reference's own numbers by
test_stats_host.py).  Counts are compared exactly.  The two calibration doubles are held to the float64 restatement with
exactly rounded sums: |logit_mean| error <= 1e-10 (n 2^-52 mean|x| is about 2e-11 at n = 4096, |x| <= 20) and |logit_std| error
<= 1e-8 (the variance's error over 2 std, std >= 0.1), for n <= 4096."""
import math

import numpy as np
import pytest

import stats_reference as ref
from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd import params as P

pytestmark = pytest.mark.gpu

INVALID = 1
FIELDS = ('pos_gt', 'neg_gt', 'pos_ge', 'neg_ge')
INTS = ('n', 'n_pos', 'n_neg', 'n_other', 'n_nan', 'n_unsaturated', 'n_fit')
SIZES = (1, 63, 64, 65, 257, 1025)          # the word, wave and workgroup edges of a 4-wave block
TABLES = (0, 1, 98, 1000, 4096)


@pytest.fixture(scope='module')
def eng(stock_weights):
    e = _lib.HipEngine(P.pr, stock_weights, n_streams=1)
    yield e
    e.close()


def predictions(rows, n, seed):
    """float32 [rows, n]: sigmoid of wide logits (|logit| <= 15), with exact 0.0, 1.0, NaN and float32(0.1) sprinkled in"""
    rng = np.random.default_rng(seed)
    p = (1 / (1 + np.exp(-rng.normal(1.0, 3.0, (rows, n)).clip(-15, 15)))).astype(np.float32)
    if n >= 63:
        for r in range(rows):
            idx = rng.permutation(n)
            p[r, idx[0:2]], p[r, idx[2:4]], p[r, idx[4:6]], p[r, idx[6:8]] = 0.0, 1.0, np.nan, np.float32(0.1)
    return p


def targets_for(n, seed, fractional=True):
    rng = np.random.default_rng(1000 + seed)
    y = (rng.random(n) < 0.5).astype(np.float32)
    if fractional and n >= 63:
        y[rng.permutation(n)[:3]] = (0.3, 0.5, 0.75)            # two of neither class, one positive that is not 1
    return y


def table(T, p, seed):
    """T non-decreasing thresholds: random ones, duplicates, values that equal a prediction exactly, 0, 1, 0.1 and a neighbour
    of 0.1 that is another float64 and the same float32"""
    rng = np.random.default_rng(2000 + seed)
    t = rng.random(T)
    special = [0.1, 0.1 + 1e-12, 0.0, 1.0] + [float(v) for v in p.reshape(-1)[:40] if v == v]
    k = min(T // 2, len(special))
    t[:k] = special[:k]
    if T >= 8:
        t[k:k + T // 8] = t[:T // 8]                            # duplicates
    return np.sort(t)


def assert_counts(got, p, y, thr, compare, what=''):
    assert got.shape == (p.shape[0], len(thr))
    for r in range(p.shape[0]):
        want = ref.counts(p[r], y, thr, compare)
        for f in FIELDS:
            assert np.array_equal(got[r][f], want[f]), (what, r, f, compare)


def assert_summary_ints(got, p, y):
    for r in range(p.shape[0]):
        want = ref.summary(p[r], y)
        assert [int(got[r][f]) for f in INTS] == [want[f] for f in INTS], r


# ---- 1. pe_stats_scores against the restatement -----------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_counts_equal_the_restatement(eng, n):
    p, y = predictions(3, n, n), targets_for(n, n)
    for T in TABLES:
        thr = table(T, p, T)
        for compare in ('f32', 'f64'):
            counts, summary = eng.stats_scores(p, y, thr, compare)
            assert_counts(counts, p, y, thr, compare, (n, T))
            assert_summary_ints(summary, p, y)


def test_the_two_compare_modes_differ_at_a_tenth(eng):
    """float32(0.1) against 0.1: not above it in float32 (equal), above it once widened (0.100000001490116...)"""
    p = np.array([[np.float32(0.1)]], dtype=np.float32)
    y = np.ones(1, dtype=np.float32)
    f32, _ = eng.stats_scores(p, y, [0.1], 'f32')
    f64, _ = eng.stats_scores(p, y, [0.1], 'f64')
    assert (int(f32[0, 0]['pos_gt']), int(f32[0, 0]['pos_ge'])) == (0, 1)
    assert (int(f64[0, 0]['pos_gt']), int(f64[0, 0]['pos_ge'])) == (1, 1)
    assert bool(np.float32(0.1) > 0.1) is False and bool(np.float64(np.float32(0.1)) > np.float64(0.1)) is True    # numpy's two answers


def test_strided_rows(eng):
    """raw[n_rows][stride] with stride > n: only the first n of a row count"""
    n, stride = 65, 100
    raw = predictions(3, stride, 5)
    y = targets_for(n, 5)
    thr = table(98, raw[:, :n], 5)
    counts, summary = _lib._stats_out(3, 98)
    rc = eng._lib.pe_stats_scores(eng._h, raw.ctypes.data, 3, stride, y.ctypes.data, n, thr.ctypes.data, 98, 0, counts.ctypes.data, summary.ctypes.data)
    assert rc == 0
    assert_counts(counts, raw[:, :n].copy(), y, thr, 'f32')
    assert_summary_ints(summary, raw[:, :n].copy(), y)


# ---- 2. the summary ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (65, 1025, 4096))
def test_calibration_summary(eng, n):
    p, y = predictions(3, n, 40 + n), targets_for(n, 40 + n)
    thr = table(98, p, 1)
    _, summary = eng.stats_scores(p, y, thr, 'f32')
    assert_summary_ints(summary, p, y)
    for r in range(3):
        want = ref.summary(p[r], y)
        assert abs(want['logit_mean']) <= 20 and want['logit_std'] >= 0.1 and want['n_fit'] > 10
        mean_err, std_err = abs(float(summary[r]['logit_mean']) - want['logit_mean']), abs(float(summary[r]['logit_std']) - want['logit_std'])
        lit = ref.literal_mu_std(np.where(np.isnan(p[r]), np.float32(0), p[r]), y)
        print('n = %d row %d: |mean - restatement| = %.3g, |std - restatement| = %.3g; float32 script: |mean| %.3g |std| %.3g'
              % (n, r, mean_err, std_err, abs(float(summary[r]['logit_mean']) - lit[0]), abs(float(summary[r]['logit_std']) - lit[1])))
        assert mean_err <= 1e-10 and std_err <= 1e-8
    # the same bits: in a second call, for a row alone, with another threshold table, without one
    again = eng.stats_scores(p, y, thr, 'f32')[1]
    assert again.tobytes() == summary.tobytes()
    for other in (table(1000, p, 2), None):
        assert eng.stats_scores(p, y, other, 'f64')[1].tobytes() == summary.tobytes()
    for r in range(3):
        assert eng.stats_scores(p[r], y, thr, 'f32')[1][0].tobytes() == summary[r].tobytes()


def test_no_calibration_sample_gives_nan(eng):
    p = predictions(2, 257, 9)
    y = np.zeros(257, dtype=np.float32)
    p[1] = 1.0                                              # row 1: positives there, every prediction saturated
    y1 = np.ones(257, dtype=np.float32)
    _, s0 = eng.stats_scores(p[0], y, [0.5])
    _, s1 = eng.stats_scores(p[1], y1, [0.5])
    for s, unsat in ((s0[0], 257 - 6), (s1[0], 0)):
        assert int(s['n_fit']) == 0 and int(s['n_unsaturated']) == unsat
        assert math.isnan(float(s['logit_mean'])) and math.isnan(float(s['logit_std']))


# ---- 3. pe_test_clips --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def clips():
    rng = np.random.default_rng(77)
    lengths = [1, 2, 1599, 1600, 24000, 24001, 30000] + [int(v) for v in rng.integers(3, 26000, 33)]
    out = [(synth.stream_pcm(300 + i, n).astype(np.float32) / np.float32(32768.0)) for i, n in enumerate(lengths)]
    assert len(out) == 40 and max(lengths) > P.pr.max_samples
    return out


def test_clips_scored_and_counted_in_one_call(stock_weights, clips):
    models = [stock_weights, synth.make_weights(13, (20,), seed=5)]
    e = _lib.HipEngine(P.pr, models, n_streams=1)
    y = targets_for(len(clips), 3, fractional=False)
    want_scores = e.score_clips(clips, P.pr.max_samples)[:, :, 0]
    thr = np.sort(np.concatenate([np.linspace(0.01, 0.99, 90), [float(v) for v in want_scores.reshape(-1)[:8]]]))
    pcm = synth.batch_pcm(1, 3)
    e.clear()
    before = [e.update(pcm[u]).copy() for u in range(3)]
    e.clear()
    got_updates = [e.update(pcm[0]).copy()]
    results = []
    for i, pass_bytes in enumerate((256 << 20, 100000, 1)):
        e.set_clip_pass_bytes(pass_bytes)
        for compare in ('f32', 'f64'):
            counts, summary, scores = e.test_clips(clips, P.pr.max_samples, y, thr, compare, return_scores=True)
            assert scores.tobytes() == want_scores.tobytes(), pass_bytes
            alone_counts, alone_summary = e.stats_scores(want_scores, y, thr, compare)
            assert counts.tobytes() == alone_counts.tobytes() and summary.tobytes() == alone_summary.tobytes()
            assert_counts(counts, want_scores, y, thr, compare)
            results.append((compare, counts.tobytes(), summary.tobytes()))
            no_scores = e.test_clips(clips, P.pr.max_samples, y, thr, compare)
            assert no_scores[2] is None and no_scores[0].tobytes() == counts.tobytes() and no_scores[1].tobytes() == summary.tobytes()
        if i < 2:                                               # the stream goes on between the clip calls
            got_updates.append(e.update(pcm[i + 1]).copy())
    for compare in ('f32', 'f64'):
        assert len({r[1:] for r in results if r[0] == compare}) == 1           # no output depends on the pass size
    assert [u.tobytes() for u in got_updates] == [u.tobytes() for u in before]      # the streams are untouched
    e.close()


# ---- 4. pe_trainer_stats_models ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_val', (33, 257))
def test_trainer_networks_over_resident_and_host_data(n_val):
    rng = np.random.default_rng(n_val)
    models = [synth.make_weights(13, (h,), seed=10 + i) for i, h in enumerate((1, 20, 32))]
    t = _lib.HipTrainer(models, 29, 13)
    x = rng.normal(0.0, 3.0, (n_val, 29, 13)).astype(np.float32)
    y = targets_for(n_val, n_val, fractional=False)
    t.set_validation(x, y)
    t.set_data(x[:20], y[:20])
    want_probs = t.evaluate_models(source='validation')[2]
    thr = np.sort(np.concatenate([np.linspace(0.0, 1.0, 90), [float(v) for v in want_probs.reshape(-1)[:8]]]))
    for compare in ('f32', 'f64'):
        counts, summary, probs = t.stats_models(thresholds=thr, compare=compare, source='validation', want_probs=True)
        assert probs.tobytes() == want_probs.tobytes()
        assert_counts(counts, want_probs, y, thr, compare)
        assert_summary_ints(summary, want_probs, y)
        host = t.stats_models(x, y, thresholds=thr, compare=compare, source='host', want_probs=True)
        assert host[2].tobytes() == t.evaluate_models(x, y)[2].tobytes()
        assert_counts(host[0], host[2], y, thr, compare)
        assert_summary_ints(host[1], host[2], y)
    counts, summary, probs = t.stats_models(thresholds=thr, source='data', want_probs=True)
    assert probs.shape == (3, 20) and probs.tobytes() == t.evaluate_models(source='data')[2].tobytes()
    assert_counts(counts, probs, y[:20], thr, 'f32')
    assert t.stats_models(thresholds=None, source='validation')[0].shape == (3, 0)
    t.close()


def test_fractional_targets_are_counted_apart_and_refused_by_name():
    from mycroft_precise_amd.train import Trainer, TrainerGroup
    from mycroft_precise_amd.model import ModelParams
    rng = np.random.default_rng(4)
    x = rng.normal(0.0, 1.0, (70, 29, 13)).astype(np.float32)
    y = targets_for(70, 4, fractional=True)
    tr = Trainer(params=ModelParams(recurrent_units=8), seed=3)
    tr.set_data(x, y, validation=True)
    counts, summary, probs = tr._t.stats_models(thresholds=[0.5], source='validation', want_probs=True)
    assert int(summary[0]['n_other']) == 2 and int(summary[0]['n_pos']) + int(summary[0]['n_neg']) == 68
    assert_counts(counts, probs, y, [0.5], 'f32')
    with pytest.raises(ValueError, match='n_other = 2'):
        tr.stats()
    tr.close()
    group = TrainerGroup([ModelParams(recurrent_units=8), ModelParams(recurrent_units=12)], seed=3)
    group._t.set_validation(x, y)
    with pytest.raises(ValueError, match='n_other = 2'):
        group.stats()
    group.close()


# ---- 5. Python, end to end ---------------------------------------------------------------------------------------------
@pytest.fixture
def keep_pr():
    keep = dict(P.pr.__dict__)
    yield
    P.pr.__dict__.clear()
    P.pr.__dict__.update(keep)


def learning_task(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (n, 29, 13)).astype(np.float32)
    y = (rng.random(n) < 0.5).astype(np.float32)
    x[y > 0, 12:20, 2:5] += np.float32(1.5)
    return x, y


def test_runner_trainers_and_calibration_end_to_end(tmp_path, clips, keep_pr):
    from mycroft_precise_amd import stats as S
    from mycroft_precise_amd.model import ModelParams
    from mycroft_precise_amd.network_runner import HipRunner, Listener
    from mycroft_precise_amd.threshold_decoder import ThresholdDecoder
    from mycroft_precise_amd.train import TrainerGroup
    x, y = learning_task(120, 1)
    xv, yv = learning_task(70, 2)
    group = TrainerGroup([ModelParams(recurrent_units=20, loss_bias=0.7), ModelParams(recurrent_units=20, loss_bias=0.4)], seeds=(5, 6))
    group.fit(x, y, batch_size=40, epochs=2, validation_data=(xv, yv))
    thr = S.graph_thresholds(ThresholdDecoder(P.pr.threshold_config, P.pr.threshold_center))
    sweeps = group.stats(thr)
    pred = group.predict(xv)
    for m, sweep in enumerate(sweeps):
        host = S.Stats(pred[m], yv.reshape(-1, 1), [])
        for j in (0, 40, 97):
            assert type(thr[j]) is float                        # (a Python float: numpy compares it in float32, compare='f32')
            assert sweep.to_dict(j) == host.to_dict(thr[j])
            assert int(sweep.num_correct[j]) == int(host.num_correct(thr[j]))
        assert sweep.false_positives().tolist() == [host.false_positives(t) for t in thr]
        assert sweep.false_negatives().tolist() == [host.false_negatives(t) for t in thr]
        fx, fy = S.roc_points(sweep)
        assert fx.shape == fy.shape == (98,)
    # calibrate candidate 0, save it, and let a fresh Listener / HipRunner decode with the fitted table
    mu_std = S.calc_threshold(sweeps[0])
    want = ref.summary(pred[0], yv)
    assert abs(mu_std[0] - want['logit_mean']) <= 1e-10 and abs(mu_std[1] - 1.2 * want['logit_std']) <= 1.2e-8
    model = str(tmp_path / 'candidate.npz')
    group.save(0, model)
    S.save_threshold(model, mu_std)
    P.pr.__dict__.update(threshold_config=((6, 4),))
    listener = Listener(model)
    assert isinstance(listener.runner, HipRunner)
    fitted = ThresholdDecoder((mu_std,), P.pr.threshold_center)
    assert [tuple(v) for v in listener.pr.threshold_config] == [mu_std]
    assert listener.threshold_decoder.cd.tobytes() == fitted.cd.tobytes()
    assert listener.threshold_decoder.decode(np.float32(0.8)) == fitted.decode(np.float32(0.8))
    # HipRunner.test_clips: one model and two, against predict_clips + Stats
    yc = targets_for(len(clips), 8, fractional=False)
    one = HipRunner(weights=group.weights[0])
    sweep, scores = one.test_clips(clips, yc, thr, return_scores=True)
    assert scores.tobytes() == one.predict_clips(clips).tobytes()
    host = S.Stats(scores, yc.reshape(-1, 1), ['clip%d' % i for i in range(len(clips))])
    assert [sweep.to_dict(j) for j in range(98)] == [host.to_dict(t) for t in thr]
    assert sorted(host.calc_filenames(False, True, thr[40]) + host.calc_filenames(False, False, thr[40]) +
                  host.calc_filenames(True, True, thr[40]) + host.calc_filenames(True, False, thr[40])) == sorted(host.filenames)
    single = S.sweep_scores(one, scores, yc, thr)
    assert single.counts.tobytes() == sweep.counts.tobytes() and single.logit_mean == sweep.logit_mean
    two = HipRunner(weights=group.weights)
    both = two.test_clips(clips, yc, thr)
    scores2 = two.predict_clips(clips)
    assert len(both) == 2 and scores2.shape == (2, len(clips), 1)
    for m in range(2):
        assert_counts(both[m].counts[np.newaxis], scores2[m].reshape(1, -1), yc, thr, 'f32')
    one.engine.close()
    two.engine.close()
    group.close()


def test_trial_reports_equal_the_host_loop(keep_pr):
    from mycroft_precise_amd import stats as S
    from mycroft_precise_amd.model import ModelParams
    from mycroft_precise_amd.network_runner import HipRunner
    from mycroft_precise_amd.train import TrainerGroup, trial_reports
    x, y = learning_task(120, 1)
    xv, yv = learning_task(70, 2)
    group = TrainerGroup([ModelParams(recurrent_units=20, loss_bias=0.7), ModelParams(recurrent_units=20, loss_bias=0.4)], seeds=(5, 6))
    group.fit(x, y, batch_size=40, epochs=2, validation_data=(xv, yv))
    noise = [synth.stream_pcm(900 + i, n).astype(np.float32) / np.float32(32768.0) for i, n in enumerate((40000, 90000, 61234))]
    runner = HipRunner(weights=group.weights)
    with pytest.raises(ValueError, match='multi-model'):
        trial_reports(group, HipRunner(weights=group.weights[0]), noise)
    reports = trial_reports(group, runner, noise, interaction_estimate=100, ambient_annoyance=1.0)
    pred = group.predict(xv)
    windows = runner.evaluate_clips(noise, 4096)
    seconds = 0.0
    for a in noise:
        seconds += len(a) / P.pr.sample_rate
    for m, report in enumerate(reports):
        p = pred[m]
        assert report['test_stats'] == S.Stats(p, yv.reshape(-1, 1), []).to_dict()
        annoyance, ww, nww, threshold, _ = ref.estimate(p[yv > 0.5], [w[m] for w in windows], seconds, 100, 1.0)
        size = 1.0 + math.exp((group._t.n_params[m] - 11000) / 10000)
        assert report['best_threshold'] == threshold
        assert report['cost_info'] == {'params_cost': size, 'annoyance': annoyance, 'ww_annoyance': ww, 'nww_annoyance': nww}
        assert report['cost'] == annoyance + size
    assert group.best('cost') == int(np.argmin([r['cost'] for r in reports]))
    assert group.best('val_loss') == int(np.argmin([h['val_loss'][-1] for h in group.histories]))
    group.close()


# ---- 6. every refusal leaves the outputs untouched ---------------------------------------------------------------------
def ptr(a):
    return None if a is None else a.ctypes.data


def test_refusals_leave_the_outputs_untouched(eng, clips):
    n, T = 65, 4
    p, y = predictions(2, n, 1), targets_for(n, 1)
    thr = np.array([0.1, 0.2, 0.2, 0.9])
    counts, summary = _lib._stats_out(2, T)
    counts.view(np.uint8)[...] = 0xA5
    summary.view(np.uint8)[...] = 0xA5
    sentinel = (counts.tobytes(), summary.tobytes())
    lib, h = eng._lib, eng._h

    def scores(raw=p, rows=2, stride=n, targets=y, n_=n, thr_=thr, T_=T, compare=0, counts_=counts, summary_=summary):
        rc = lib.pe_stats_scores(h, ptr(raw), rows, stride, ptr(targets), n_, ptr(thr_), T_, compare, ptr(counts_), ptr(summary_))
        assert (counts.tobytes(), summary.tobytes()) == sentinel
        return rc

    bad_target, nan_target = y.copy(), y.copy()
    bad_target[7], nan_target[64] = 1.5, np.nan
    assert lib.pe_stats_scores(None, ptr(p), 2, n, ptr(y), n, ptr(thr), T, 0, ptr(counts), ptr(summary)) == INVALID
    for kw in (dict(raw=None), dict(targets=None), dict(summary_=None), dict(counts_=None), dict(thr_=None), dict(n_=0), dict(n_=-3),
               dict(rows=0), dict(rows=17), dict(stride=n - 1), dict(thr_=np.array([0.1, 0.3, 0.2, 0.9])),
               dict(thr_=np.array([0.1, np.nan, 0.2, 0.9])), dict(T_=-1), dict(T_=4097), dict(compare=2), dict(compare=-1),
               dict(targets=bad_target), dict(targets=nan_target), dict(targets=-y - 0.25)):
        assert scores(**kw) == INVALID, kw
        assert eng._lib.pe_last_error(h)
    assert scores(T_=0, thr_=None, counts_=None, summary_=summary.copy()) == 0            # no table: no counts wanted

    # pe_test_clips: the same request checks, and what pe_score_clips refuses
    few = clips[:5]
    audio, offsets, fmt = eng._clips(few)
    yc = np.array([1, 0, 1, 0, 1], dtype=np.float32)
    out = np.full((1, 5), 7.0, dtype=np.float32)
    counts1, summary1 = _lib._stats_out(1, T)
    counts1.view(np.uint8)[...] = 0xA5
    summary1.view(np.uint8)[...] = 0xA5
    sentinel1 = (counts1.tobytes(), summary1.tobytes(), out.tobytes())

    def clips_call(audio_=audio, offsets_=offsets, n_=5, targets=yc, thr_=thr, T_=T, compare=0, counts_=counts1, summary_=summary1, out_=out):
        rc = lib.pe_test_clips(h, ptr(audio_), fmt, ptr(offsets_), n_, 0, ptr(targets), ptr(thr_), T_, compare, ptr(counts_), ptr(summary_), ptr(out_))
        assert (counts1.tobytes(), summary1.tobytes(), out.tobytes()) == sentinel1
        return rc

    empty = offsets.copy()
    empty[2] = empty[1]
    for kw in (dict(audio_=None), dict(offsets_=None), dict(targets=None), dict(summary_=None), dict(counts_=None), dict(thr_=None),
               dict(n_=-1), dict(offsets_=empty), dict(thr_=np.array([0.5, 0.4, 0.6, 0.7])), dict(thr_=np.array([np.nan, 0.4, 0.6, 0.7])),
               dict(T_=4097), dict(T_=-1), dict(compare=5), dict(targets=np.array([1, 0, 2, 0, 1], dtype=np.float32)),
               dict(targets=np.array([1, 0, np.nan, 0, 1], dtype=np.float32))):
        assert clips_call(**kw) == INVALID, kw
    assert clips_call(n_=0) == 0                                   # nothing to do, nothing written

    # pe_trainer_stats_models
    models = [synth.make_weights(13, (h_,), seed=3 + h_) for h_ in (4, 8)]
    t = _lib.HipTrainer(models, 29, 13)
    x = np.random.default_rng(0).normal(0.0, 1.0, (9, 29, 13)).astype(np.float32)
    yt = np.array([1, 0, 1, 0, 1, 0, 1, 0, 1], dtype=np.float32)
    probs = np.full((2, 9), 7.0, dtype=np.float32)
    sentinel2 = (counts.tobytes(), summary.tobytes(), probs.tobytes())

    def trainer_call(source=0, feats=x, targets=yt, n_=9, thr_=thr, T_=T, compare=0, counts_=counts, summary_=summary):
        rc = lib.pe_trainer_stats_models(t._h, source, ptr(feats), ptr(targets), n_, ptr(thr_), T_, compare, ptr(counts_), ptr(summary_), ptr(probs))
        assert (counts.tobytes(), summary.tobytes(), probs.tobytes()) == sentinel2
        return rc

    assert lib.pe_trainer_stats_models(None, 0, ptr(x), ptr(yt), 9, ptr(thr), T, 0, ptr(counts), ptr(summary), ptr(probs)) == INVALID
    for kw in (dict(source=1), dict(source=2), dict(source=3), dict(feats=None), dict(targets=None), dict(n_=0), dict(summary_=None),
               dict(counts_=None), dict(thr_=None), dict(thr_=np.array([0.5, 0.4, 0.6, 0.7])), dict(thr_=np.array([0.5, np.nan, 0.6, 0.7])),
               dict(T_=4097), dict(compare=2), dict(targets=yt + 0.5)):
        assert trainer_call(**kw) == INVALID, kw
        assert b'pe_trainer_stats_models' in lib.pe_trainer_last_error(t._h), kw
    assert (counts.tobytes(), summary.tobytes()) == sentinel
    t.close()
