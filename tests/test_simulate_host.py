"""CPU: the surface of the many-recordings simulation (pe_evaluate_clips / pe_simulate_*) that needs no device -- the ABI
table and the header, the report arithmetic of mycroft_precise_amd.simulate.Metric, the default thresholds."""
import os
import re

import numpy as np
import pytest

from conftest import REPO
from mycroft_precise_amd import _lib
from mycroft_precise_amd import simulate as S

NEW = {'pe_evaluate_clips_layout': 5, 'pe_evaluate_clips': 8, 'pe_simulate_scores': 13, 'pe_simulate_clips': 16}


def test_new_entry_points_are_declared_and_bound():
    text = open(os.path.join(REPO, 'include', 'precise_engine.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(pe_[a-z_0-9]+)\s*\(', text))          # (the expression of test_abi.py)
    for name, n_args in NEW.items():
        assert name in declared
        assert len(_lib.EXPORTS[name][1]) == n_args                      # handle + the arguments of the header
        proto = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, text).group(1)
        assert len(proto.split(',')) == n_args, name
    assert sorted(_lib.EXPORTS) == sorted(declared)
    assert _lib.ABI_VERSION == 8 and re.search(r'#define\s+PE_ABI_VERSION\s+8\b', text)
    for name in ('evaluate_clips_layout', 'evaluate_clips', 'simulate_scores', 'simulate_clips'):
        assert callable(getattr(_lib.HipEngine, name))
    from mycroft_precise_amd.network_runner import HipRunner
    assert callable(HipRunner.evaluate_clips) and callable(HipRunner.simulate)


def test_metric_struct_matches_the_header():
    text = open(os.path.join(REPO, 'include', 'precise_engine.h')).read()
    body = re.search(r'typedef struct pe_sim_metric \{(.*?)\} pe_sim_metric;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = re.findall(r'(int64_t|double)\s+(\w+);', body)
    assert [n for _, n in fields] == list(_lib.SIM_METRIC.names) == ['n_windows', 'activated_chunks', 'activations', 'activation_sum']
    assert [{'int64_t': '<i8', 'double': '<f8'}[t] for t, _ in fields] == [_lib.SIM_METRIC[n].str for n in _lib.SIM_METRIC.names]
    assert _lib.SIM_METRIC.itemsize == 32


def test_metric_arithmetic_and_report():
    # six hours of audio at the stock 16 kHz in chunks of 4096 samples: 84 375 chunks
    m = S.Metric(chunk_size=4096, seconds=21600.0, activated_chunks=30, activations=3, activation_sum=168.75)
    assert m.days == 0.25
    assert m.chunks == 21600.0 * 16000 / 4096 == 84375.0
    assert m.info_string('a.wav') == ('=== a.wav ===\n'
                                      'Hours: 6.00\n'
                                      'Activations / Day: 12.00\n'
                                      'Activated Chunks / Day: 120.00\n'
                                      'Average Activation (*100): 0.20')
    total = S.Metric(chunk_size=4096)
    assert (total.seconds, total.activated_chunks, total.activations, total.activation_sum) == (0.0, 0, 0, 0.0)
    total.add(m)
    total.add(S.Metric(chunk_size=4096, seconds=64800.0, activated_chunks=2, activations=1, activation_sum=0.25))
    assert (total.seconds, total.activated_chunks, total.activations, total.activation_sum) == (86400.0, 32, 4, 169.0)
    assert total.days == 1.0 and total.chunks == 337500.0
    assert total.info_string('Total').splitlines() == ['=== Total ===', 'Hours: 24.00', 'Activations / Day: 4.00',
                                                        'Activated Chunks / Day: 32.00', 'Average Activation (*100): 0.05']
    # a metric does not change the one it was added to afterwards, and chunk_size scales the chunk count alone
    assert m.seconds == 21600.0
    assert S.Metric(chunk_size=2048, seconds=1.0).chunks == 16000 / 2048
    with pytest.raises(ZeroDivisionError):              # nothing simulated: the reference's report divides by zero days as well
        S.Metric(chunk_size=4096).info_string('empty')


def test_default_thresholds():
    thr = S.default_thresholds()
    assert thr.shape == (1000,) and thr.dtype == np.float64
    x = np.linspace(-20, 20, 1000)
    assert np.array_equal(thr, 1 / (1 + np.exp(-x)))
    assert np.all(np.diff(thr) >= 0) and not np.isnan(thr).any()         # what pe_simulate_* asks of a table
    assert thr[0] == 1 / (1 + np.exp(20.0)) and 0 < thr[0] < 3e-9 and thr[-1] < 1.0 and 1 - thr[-1] < 3e-9
    assert abs(thr[499] + thr[500] - 1) < 1e-15                           # symmetric about 0.5
    assert thr.size <= 4096


def test_empty_recordings_are_skipped():
    kept = S._recordings([np.zeros(0), np.ones(3), np.zeros(0, np.float32), np.ones(2, np.float32)])
    assert [a.size for a in kept] == [3, 2]


# ---- the script itself: tests/golden/simulate.npz (tools/make_script_fixtures.py) ---------------------------------------------
SIM_CHUNKS = (1024, 2048, 4096)


@pytest.fixture(scope='module')
def sim_fixture():
    from conftest import golden
    from oracle import listener as ol
    g = golden('simulate.npz')
    off = g['offsets']
    audios = [g['pcm'][a:b].astype(np.float32) / float(np.iinfo(np.int16).max) for a, b in zip(off[:-1], off[1:])]
    feats = [ol.vectorize_raw(a, ol.Params()) for a in audios]           # once: every chunk size windows the same frames
    return g, audios, feats


def restated_predictions(feats, weights, hop_frames):
    """SimulateScript.evaluate (simulate.py:92-104) per recording; no window: an empty array"""
    from oracle import keras_gru
    out = []
    for f in feats:
        x = [f[i - 29:i] for i in range(29, len(f), hop_frames)]
        out.append(keras_gru.predict(np.array(x), weights).reshape(-1) if x else np.zeros(0, np.float32))
    return out


@pytest.mark.parametrize('C', SIM_CHUNKS)
def test_restated_metrics_and_report_equal_the_scripts_own(sim_fixture, stock_weights, C):
    """SimulateScript.run itself (evaluate, a fresh TriggerDetector per file, Metric, Metric.add, info_string) over recordings
    with 0, 1, 63, 64 and 65 predictions: predictions, counts, sums and the printed report."""
    from test_gpu_parity import TOL_RAW
    from test_simulate import host_metric
    g, audios, feats = sim_fixture
    k = '_%d' % C
    threshold, woff = float(g['threshold']), g['window_offsets' + k]
    want = [g['predictions' + k][a:b] for a, b in zip(woff[:-1], woff[1:])]
    counts = np.diff(woff).tolist()
    assert counts[:2] == [0, 1] and any(counts[i:i + 3] == [63, 64, 65] for i in range(len(counts)))
    flat = g['predictions' + k].astype(np.float64)
    assert threshold != 0.5 and min(np.abs(flat - threshold).min(), np.abs(flat - (1.0 - threshold)).min()) > TOL_RAW
    hop_frames = C // 800                                                   # chunk_size // hop_samples (simulate.py:96)
    got = restated_predictions(feats, stock_weights, hop_frames)
    assert [len(p) for p in got] == counts and all(np.array_equal(a, b) for a, b in zip(got, want))        # (as test_oracle.py)
    # the wrong readings: a window stride of hop_frames +- 1 fails against the fixture
    for wrong in (hop_frames + 1, hop_frames - 1):
        if wrong >= 1:
            other = restated_predictions(feats, stock_weights, wrong)
            assert [len(p) for p in other] != counts or not all(np.array_equal(a, b) for a, b in zip(other, want))

    rows = np.zeros(len(audios), dtype=_lib.SIM_METRIC)
    hot = []
    for r, p in enumerate(want):
        n, chunks, acts, fsum = host_metric(p, threshold, threshold, 0, C)
        assert (n, chunks, acts) == (counts[r], int(g['activated_chunks' + k][r]), int(g['activations' + k][r])), r
        # the script's sum is numpy's float32 sum of the float32 predictions: n - 1 float32 additions from the exact one
        assert abs(float(g['activation_sum' + k][r]) - fsum) <= n * 2.0 ** -24 * fsum, r
        rows[r] = (n, chunks, acts, fsum)
        hot.append(int((p.astype(np.float64) > 1.0 - threshold).sum()))
    assert any(h > a >= 1 for h, a in zip(hot, g['activations' + k].tolist()))      # a run of activated chunks cut by the re-arm
    assert g['activations' + k].max() >= 2 and (g['activated_chunks' + k] != np.array(hot)).any()          # `> t` is not `> 1 - t`
    assert np.array_equal(g['seconds' + k], np.array([len(a) / 16000 for a in audios]))

    # the report from the fixture's own numbers: Metric, add and info_string
    total = S.Metric(C)
    names = ['rec%02d.wav' % r for r in range(len(audios))]
    for r, name in enumerate(names):
        m = S.Metric(C, float(g['seconds' + k][r]), int(g['activated_chunks' + k][r]), int(g['activations' + k][r]), float(g['activation_sum' + k][r]))
        assert m.info_string(name) == str(g['file_strings' + k][r])
        total.add(m)
    assert (total.seconds, total.activated_chunks, total.activations) == tuple(g['total' + k][:3])
    assert abs(total.activation_sum - g['total' + k][3]) <= len(flat) * 2.0 ** -24 * g['total' + k][3]
    assert total.info_string('Total') == str(g['total_string' + k])

    # simulate_recordings over a runner that returns the restated rows: the float64 sums print the same report wherever a
    # figure has room for them
    class Runner:
        def simulate(self, recs, chunk_size, thr):
            assert chunk_size == C and thr == threshold and len(recs) == len(audios)
            return rows, None, None
    metrics, total = S.simulate_recordings(Runner(), audios, chunk_size=C, threshold=threshold)
    safe = g['string_safe' + k]
    assert bool(g['total_string_safe' + k]) and 2 * int(safe.sum()) > len(safe)
    for r, (m, name) in enumerate(zip(metrics, names)):
        lines, want_lines = m.info_string(name).splitlines(), str(g['file_strings' + k][r]).splitlines()
        assert lines[:4] == want_lines[:4] and (not safe[r] or lines == want_lines), r
    assert total.info_string('Total') == str(g['total_string' + k])
