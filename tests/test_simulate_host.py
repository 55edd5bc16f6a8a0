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
