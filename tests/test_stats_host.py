"""CPU: ``stats.Stats``, ``graph_thresholds``, ``annoyance.estimate`` and the host ``calc_threshold`` against what the reference's
own code computed (tests/golden/stats.npz, written by tools/make_stats_fixture.py); the restatement the GPU tests trust
(stats_reference.py) against the same file; the header, the ctypes records and the refusals ``_lib`` makes before any call."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import stats_reference as ref
from conftest import REPO, golden
from mycroft_precise_amd import _lib, annoyance, simulate
from mycroft_precise_amd import stats as S
from mycroft_precise_amd.threshold_decoder import ThresholdDecoder

SETS = ('a', 'b')
METRICS = ('true_pos', 'true_neg', 'false_pos', 'false_neg')


@pytest.fixture(scope='module')
def g():
    return golden('stats.npz')


def same_bits(got, want):
    return np.asarray(got, dtype=np.float64).tobytes() == np.asarray(want, dtype=np.float64).tobytes()


def make_stats(g, key):
    return S.Stats(g[key + '_outputs'], g[key + '_targets'], [str(f) for f in g[key + '_filenames']])


@pytest.mark.parametrize('key', SETS)
def test_stats_reproduces_the_reference(g, key):
    stats = make_stats(g, key)
    thresholds = [float(t) for t in g[key + '_thresholds']]
    assert len(stats) == int(g[key + '_len']) == {'a': 65, 'b': 2000}[key]
    assert (stats.num_positives, stats.num_negatives) == (int(g[key + '_num_positives']), int(g[key + '_num_negatives']))
    dicts = [stats.to_dict(t) for t in thresholds]
    for name in METRICS:
        assert [d[name] for d in dicts] == g[key + '_' + name].tolist(), name
    assert [stats.to_dict()[k] for k in METRICS] == g[key + '_default_dict'].tolist()
    assert [int(stats.num_correct(t)) for t in thresholds] == g[key + '_num_correct'].tolist()
    assert [int(stats.num_incorrect(t)) for t in thresholds] == g[key + '_num_incorrect'].tolist()
    assert same_bits([stats.accuracy(t) for t in thresholds], g[key + '_accuracy'])
    assert same_bits([stats.false_positives(t) for t in thresholds], g[key + '_false_positives'])
    assert same_bits([stats.false_negatives(t) for t in thresholds], g[key + '_false_negatives'])
    names = [str(f) for f in g[key + '_filenames']]
    for tag, t in (('half', 0.5), ('equal', float(g[key + '_equal_threshold']))):
        assert stats.counts_str(t) == str(g['%s_counts_str_%s' % (key, tag)])
        assert stats.summary_str(t) == str(g['%s_summary_str_%s' % (key, tag)])
        seen = 0
        for right in (True, False):
            for fired in (True, False):
                want = [names[i] for i in g['%s_files_%s_%d%d' % (key, tag, right, fired)]]
                assert stats.calc_filenames(right, fired, t) == want
                assert all(S.Stats.matches_sample(stats.outputs[names.index(f)], stats.targets[names.index(f)], t, right, fired) for f in want)
                seen += len(want)
        assert seen == len(stats)
    again = S.Stats.from_np_dict(stats.to_np_dict())
    assert again.to_dict(0.5) == stats.to_dict(0.5) and list(again.filenames) == names


@pytest.mark.parametrize('key', SETS)
def test_one_golden_threshold_equals_a_prediction(g, key):
    """... so that > (calc_metric) and >= (num_correct) part ways there, in the reference's numbers and in the restatement"""
    p, y, t = g[key + '_outputs'], g[key + '_targets'], float(g[key + '_equal_threshold'])
    assert (p == np.float32(t)).any() and np.float32(t) == t
    j = g[key + '_thresholds'].tolist().index(t)
    fired = int(g[key + '_true_pos'][j] + g[key + '_false_pos'][j])
    assert int((p >= t).sum()) > fired == int((p > t).sum())
    c = ref.counts(p, y, [t], 'f32')
    assert c['pos_ge'][0] + c['neg_ge'][0] > c['pos_gt'][0] + c['neg_gt'][0] == fired


@pytest.mark.parametrize('key', SETS)
def test_restatement_reproduces_the_reference(g, key):
    p, y = g[key + '_outputs'], g[key + '_targets']
    for j, t in enumerate(g[key + '_thresholds'].tolist()):
        c = ref.confusion(p, y, t)
        for name in METRICS:
            assert c[name] == int(g[key + '_' + name][j]), (name, t)
        assert c['num_correct'] == int(g[key + '_num_correct'][j]), t
    s = ref.summary(p, y)
    assert (s['n'], s['n_pos'], s['n_neg'], s['n_other'], s['n_nan']) == \
        (len(p), int(g[key + '_num_positives']), int(g[key + '_num_negatives']), 0, 0)
    assert s['n_unsaturated'] == len(p) - 4 and s['n_fit'] == s['n_pos'] - 2            # two exact 0.0 and two exact 1.0, one of each positive
    # the float64 contract against the script's float32 evaluation: close (float32 logarithms of values up to e^20), not equal
    mu, std = g[key + '_mu_std'][0], g[key + '_mu_std'][1] / float(g['smoothing'])
    assert abs(s['logit_mean'] - mu) < 1e-5 and abs(s['logit_std'] - std) < 1e-5
    assert abs(s['logit_mean']) <= 20 and s['logit_std'] >= 0.1
    # ... and the literal restatement is the script's, bit for bit
    lit_mu, lit_std = ref.literal_mu_std(p, y)
    assert same_bits([lit_mu, lit_std * float(g['smoothing'])], g[key + '_mu_std'])
    # the annoyance estimate
    seconds, noise = 0.0, []
    first = 0
    for n, samples in zip(g['noise_windows'], g['noise_samples']):
        seconds += int(samples) / int(g['sample_rate'])
        noise.append(g['noise_predictions'][first:first + n])
        first += n
    *est, ww = ref.estimate(p[y > 0.5], noise, seconds, float(g['interaction_estimate']), float(g['ambient_annoyance']))
    assert same_bits(ww, g[key + '_ww_annoyances']) and same_bits(est, g[key + '_estimate'])
    assert same_bits(ref.annoyance_thresholds(), g['annoyance_thresholds'])


def test_graph_thresholds_reproduce_the_reference(g):
    decoder = ThresholdDecoder([tuple(v) for v in g['threshold_config']], float(g['threshold_center']))
    got = S.graph_thresholds(decoder)
    assert len(got) == 98 and same_bits(got, g['graph_thresholds'])
    assert np.all(np.diff(got) >= 0)                    # a table the device calls accept as it is
    assert len(S.graph_thresholds(decoder, 10)) == 8


@pytest.mark.parametrize('key', SETS)
def test_annoyance_estimate_reproduces_the_reference(g, key):
    p, y = g[key + '_outputs'], g[key + '_targets']
    thr = simulate.default_thresholds()
    assert same_bits(thr, g['annoyance_thresholds'])
    ww_buckets = ref.buckets(p[y > 0.5], thr)            # what pos_gt of an F64 sweep holds
    nww_buckets = ref.buckets(g['noise_predictions'], thr).astype(np.float64)
    seconds = 0.0
    for samples in g['noise_samples']:
        seconds += int(samples) / int(g['sample_rate'])
    assert same_bits(annoyance.ww_annoyances(ww_buckets, int((y > 0.5).sum()), float(g['interaction_estimate'])), g[key + '_ww_annoyances'])
    est = annoyance.estimate(ww_buckets, int((y > 0.5).sum()), nww_buckets, seconds, float(g['interaction_estimate']),
                             float(g['ambient_annoyance']))
    assert isinstance(est, annoyance.AnnoyanceEstimate) and est._fields == ('annoyance', 'ww_annoyance', 'nww_annoyance', 'threshold')
    assert same_bits(list(est), g[key + '_estimate'])
    with pytest.raises(ValueError):
        annoyance.estimate(ww_buckets[:10], 5, nww_buckets, seconds)


@pytest.mark.parametrize('key', SETS)
def test_host_calc_threshold_reproduces_the_script(g, key):
    stats = make_stats(g, key)
    got = S.calc_threshold(stats, float(g['smoothing']))
    assert same_bits(got, g[key + '_mu_std'])
    assert S.calc_threshold(S.Stats(np.array([[0.0], [1.0]], np.float32), np.array([[0.0], [1.0]], np.float32), ['a', 'b'])) is None


def test_sweep_arithmetic_and_refusal():
    """a Sweep built from device records by hand: the derived arrays, the rates, to_dict -- and n_other refused by name"""
    counts = np.zeros(2, dtype=_lib.STATS_COUNT)
    counts['pos_gt'], counts['neg_gt'], counts['pos_ge'], counts['neg_ge'] = [3, 1], [2, 0], [4, 1], [2, 1]
    summary = np.zeros(1, dtype=_lib.STATS_SUMMARY)[0]
    summary['n'], summary['n_pos'], summary['n_neg'], summary['n_unsaturated'], summary['n_fit'] = 9, 4, 5, 9, 4
    summary['logit_mean'], summary['logit_std'] = 1.5, 2.0
    sweep = S.Sweep([0.25, 0.75], counts, summary)
    assert sweep.true_pos.tolist() == [3, 1] and sweep.false_pos.tolist() == [2, 0]
    assert sweep.false_neg.tolist() == [1, 3] and sweep.true_neg.tolist() == [3, 5]
    assert sweep.num_correct.tolist() == [4 + 3, 1 + 4] and len(sweep) == 9
    assert sweep.false_positives().tolist() == [2 / 5, 0.0] and sweep.false_negatives().tolist() == [1 / 4, 3 / 4]
    assert sweep.to_dict(1) == {'true_pos': 1, 'true_neg': 5, 'false_pos': 0, 'false_neg': 3}
    x, y = S.roc_points(sweep)
    assert x.tolist() == sweep.false_positives().tolist() and y.tolist() == sweep.false_negatives().tolist()
    assert S.calc_threshold(sweep, 1.2) == (1.5, 2.0 * 1.2)
    summary['n_unsaturated'] = 0
    assert S.calc_threshold(S.Sweep([0.25, 0.75], counts, summary)) is None
    summary['n_other'] = 2
    with pytest.raises(ValueError, match='n_other = 2'):
        S.Sweep([0.25, 0.75], counts, summary)


def test_save_threshold_writes_the_params_a_listener_reads(tmp_path):
    from mycroft_precise_amd import params as P
    keep = dict(P.pr.__dict__)
    try:
        model = str(tmp_path / 'model.npz')
        S.save_threshold(model, (1.25, 2.5))
        assert P.pr.threshold_config == ((1.25, 2.5),)
        P.pr.__dict__.update(threshold_config=((6, 4),))
        assert [tuple(v) for v in P.inject_params(model).threshold_config] == [(1.25, 2.5)]
    finally:
        P.pr.__dict__.clear()
        P.pr.__dict__.update(keep)


def test_header_carries_the_statistics_abi():
    header = open(os.path.join(REPO, 'include', 'precise_engine.h')).read()
    flat = re.sub(r'\s+', ' ', header)
    assert '#define PE_ABI_VERSION 8' in header and _lib.ABI_VERSION == 8
    assert '#define PE_STATS_COMPARE_F32 0' in header and '#define PE_STATS_COMPARE_F64 1' in header
    assert 'typedef struct pe_stats_count { /* one (row, threshold) */ int64_t pos_gt, neg_gt, pos_ge, neg_ge; } pe_stats_count;' in flat
    assert ('typedef struct pe_stats_summary { /* one row */ int64_t n, n_pos, n_neg, n_other, n_nan, n_unsaturated, n_fit; '
            'double logit_mean, logit_std; } pe_stats_summary;') in flat
    for proto in (
            'int pe_stats_scores(pe_engine* e, const float* raw_host, int32_t n_rows, int64_t stride, const float* targets_host, int64_t n, '
            'const double* thresholds, int32_t n_thresholds, int32_t compare, pe_stats_count* counts_out, pe_stats_summary* summary_out);',
            'int pe_test_clips(pe_engine* e, const void* audio_host, int32_t sample_format, const int64_t* offsets_host, int32_t n_clips, '
            'int64_t max_samples, const float* targets_host, const double* thresholds, int32_t n_thresholds, int32_t compare, '
            'pe_stats_count* counts_out, pe_stats_summary* summary_out, float* out_host);',
            'int pe_trainer_stats_models(pe_trainer* t, int32_t source, const float* feats_host, const float* targets_host, int32_t n, '
            'const double* thresholds, int32_t n_thresholds, int32_t compare, pe_stats_count* counts_out, pe_stats_summary* summary_out, '
            'float* probs_out);'):
        assert proto in flat, proto
    for name, n_args in (('pe_stats_scores', 11), ('pe_test_clips', 13), ('pe_trainer_stats_models', 11)):
        assert len(_lib.EXPORTS[name][1]) == n_args


def test_ctypes_records_have_the_c_sizes():
    assert ctypes.sizeof(_lib.PeStatsCount) == _lib.STATS_COUNT.itemsize == 32
    assert ctypes.sizeof(_lib.PeStatsSummary) == _lib.STATS_SUMMARY.itemsize == 72
    assert _lib.STATS_COUNT.names == ('pos_gt', 'neg_gt', 'pos_ge', 'neg_ge')
    assert _lib.STATS_SUMMARY.names == ('n', 'n_pos', 'n_neg', 'n_other', 'n_nan', 'n_unsaturated', 'n_fit', 'logit_mean', 'logit_std')
    assert [_lib.STATS_SUMMARY.fields[n][1] for n in _lib.STATS_SUMMARY.names] == list(range(0, 72, 8))


def test_lib_refuses_a_bad_request_before_any_call():
    thr, code = _lib.stats_request([0.1, 0.1, 0.5], 'f64')
    assert thr.dtype == np.float64 and thr.tolist() == [0.1, 0.1, 0.5] and code == 1
    assert _lib.stats_request(0.5, 'f32')[0].tolist() == [0.5] and _lib.stats_request(None, 'f32')[0].size == 0
    for bad, what in (([0.5, 0.4], 'decrease at 1'), ([0.1, float('nan')], r'thresholds\[1\] is NaN'), (np.zeros(4097), 'at most 4096'),
                      (np.zeros((2, 2)), '1-D')):
        with pytest.raises(ValueError, match=what):
            _lib.stats_request(bad, 'f32')
    for bad in ('f16', 0, None):
        with pytest.raises(ValueError, match='compare'):
            _lib.stats_request([0.5], bad)

    # ... and the wrappers call it before they touch their handle: an object without one gets the ValueError, not an AttributeError
    class NoHandle:
        pass
    with pytest.raises(ValueError, match='decrease'):
        _lib.HipEngine.stats_scores(NoHandle(), np.zeros(3, np.float32), np.zeros(3), [0.5, 0.4])
    with pytest.raises(ValueError, match='compare'):
        _lib.HipEngine.test_clips(NoHandle(), [np.zeros(3)], 0, np.zeros(1), [0.5], 'f16')
    with pytest.raises(ValueError, match='NaN'):
        _lib.HipTrainer.stats_models(NoHandle(), thresholds=[float('nan')], source='validation')


def test_compat_aliases_resolve():
    code = ("from precise.stats import Stats\n"
            "from precise.annoyance_estimator import AnnoyanceEstimate\n"
            "import precise.stats, precise.annoyance_estimator, mycroft_precise_amd.stats, mycroft_precise_amd.annoyance\n"
            "assert precise.stats is mycroft_precise_amd.stats and precise.annoyance_estimator is mycroft_precise_amd.annoyance\n"
            "assert Stats([[0.75]], [[1.0]], ['a']).to_dict() == {'true_pos': 1, 'true_neg': 0, 'false_pos': 0, 'false_neg': 0}\n"
            "print('aliases ok')\n")
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.join(REPO, 'compat'), REPO] + ([env['PYTHONPATH']] if env.get('PYTHONPATH') else []))
    env['PYTHONDONTWRITEBYTECODE'] = '1'
    res = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and 'aliases ok' in res.stdout, res.stdout + res.stderr


def test_group_best_by_cost_needs_reports():
    from mycroft_precise_amd.train import TrainerGroup, params_cost
    group = TrainerGroup.__new__(TrainerGroup)
    with pytest.raises(ValueError, match='trial_reports'):
        group.best('cost')
    group.reports = [{'cost': 3.0}, {'cost': 1.5}, {'cost': 2.0}]
    assert group.best('cost') == 1
    with pytest.raises(ValueError, match='val_loss'):
        group.best('val_loss')
    assert params_cost(11000) == 2.0 and params_cost(1000) == 1.0 + math.exp(-1.0)
