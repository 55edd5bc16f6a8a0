"""CPU: what sampled training does on the host -- the header and the ctypes declarations of its calls, the sample hash, the
samples file, the eligible mask and the metrics line."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np

import sampled_reference as ref
from conftest import REPO
from mycroft_precise_amd import _lib, train
from mycroft_precise_amd.util import calc_sample_hash

CALLS = ('pe_trainer_evaluate_indices', 'pe_trainer_sample_reset', 'pe_trainer_sample_choose', 'pe_trainer_sample_selected')


def header():
    with open(os.path.join(REPO, 'include', 'precise_engine.h')) as f:
        return f.read()


def test_header_declares_the_calls_and_abi_stays_8():
    text = header()
    for name in CALLS:
        assert re.search(r'^int %s\(pe_trainer\* t, ' % name, text, re.M), name
    assert re.search(r'^#define PE_ABI_VERSION 8$', text, re.M)
    defines = dict(re.findall(r'^#define (PE_SAMPLE_\w+) (\d+)', text, re.M))
    assert defines == {'PE_SAMPLE_ORDER_INDEX': '0', 'PE_SAMPLE_ORDER_ERROR': '1', 'PE_SAMPLE_MAX_NEW': '1024', 'PE_SAMPLE_BLOCK_ROWS': '2048'}
    assert _lib.SAMPLE_ORDER == {'index': 0, 'error': 1}
    assert (_lib.SAMPLE_MAX_NEW, _lib.SAMPLE_BLOCK_ROWS) == (1024, 2048)
    body = re.search(r'typedef struct pe_sample_report \{(.*?)\} pe_sample_report;', text, re.S).group(1)
    fields = re.findall(r'int64_t (\w+);', body)
    assert fields == [name for name, _ in _lib.PeSampleReport._fields_] == ['n', 'n_correct', 'n_failed', 'n_remaining', 'n_added', 'n_selected']
    assert ctypes.sizeof(_lib.PeSampleReport) == 48


def test_lib_declares_the_calls_with_the_header_arity():
    text = header()
    for name in CALLS + ('pe_trainer_n_selected',):
        restype, argtypes = _lib.EXPORTS[name]
        declared = re.search(r'^int %s\((.*?)\);' % name, text, re.M | re.S).group(1)
        declared = re.sub(r'/\*.*?\*/', '', declared, flags=re.S)
        assert restype is ctypes.c_int and len(argtypes) == len(declared.split(',')), name
    for method in ('evaluate_indices', 'sample_reset', 'sample_choose', 'sample_selected'):
        assert callable(getattr(_lib.HipTrainer, method))


def test_calc_sample_hash_is_md5_of_input_then_target_bytes():
    rng = np.random.default_rng(3)
    inp, outp = rng.normal(size=(29, 13)), np.array([1.0])
    assert inp.dtype == outp.dtype == np.float64
    want = hashlib.md5(inp.tobytes() + outp.tobytes()).hexdigest()
    assert calc_sample_hash(inp, outp) == want == ref.calc_sample_hash(inp, outp)
    assert calc_sample_hash(inp, np.array([0.0])) != want                   # only the target differs
    assert calc_sample_hash(inp.astype(np.float32), outp) != want           # the bytes as they are, not a cast of them
    assert train.sample_hashes(np.stack([inp, inp]), np.array([[1.0], [0.0]])) == [want, calc_sample_hash(inp, np.array([0.0]))]


def test_eligible_mask_marks_the_last_occurrence_only():
    hashes = ['a', 'b', 'a', 'c', 'b', 'a', 'd']
    assert train.eligible_mask(hashes).tolist() == [False, False, False, True, True, True, True]
    hash_to_ind = {h: i for i, h in enumerate(hashes)}
    assert sorted(hash_to_ind.values()) == np.flatnonzero(train.eligible_mask(hashes)).tolist()
    assert train.eligible_mask(['x']).tolist() == [True] and train.eligible_mask([]).size == 0


def test_samples_file_round_trip_drops_unknown_hashes(tmp_path, capsys):
    path = str(tmp_path / 'model.samples.json')
    hash_to_ind = {'h0': 0, 'h1': 1, 'h2': 2}
    train.write_samples_file(path, ['h2', 'h0'])
    with open(path) as f:
        assert json.load(f) == ['h2', 'h0']
    assert train.read_samples_file(path) == ['h2', 'h0']
    train.write_samples_file(path, ['h2', 'gone', 'h0', 'h2'])
    found = train.read_samples_file(path)
    assert found == ['h2', 'gone', 'h0']                                    # each hash once, in file order
    assert train.known_samples(found, hash_to_ind) == ['h2', 'h0']
    assert capsys.readouterr().out == 'Missing hash: gone\n'
    assert train.read_samples_file(str(tmp_path / 'absent.json')) == []


def test_samples_file_reads_one_hash_per_line(tmp_path):
    path = str(tmp_path / 'lines.txt')
    with open(path, 'w') as f:
        f.write('h1\n\n  h0  \nh1\n')
    assert train.read_samples_file(path) == ['h1', 'h0']
    with open(path, 'w') as f:
        f.write('')
    assert train.read_samples_file(path) == []


def test_metrics_line_is_formatted_as_the_script_formats_it():
    n, n_selected, n_correct = 60, 5, 41
    predicted = np.zeros((n, 1), dtype=np.float32)
    targets = np.zeros((n, 1))
    targets[:n - n_correct] = 1.0
    correct = float(sum((predicted > 0.5) == (targets > 0.5))[0] / len(targets))                      # train_sampled.py:55
    want = '{}\t{}'.format(n_selected / len(targets), correct)                                         # train_sampled.py:59
    assert train.metrics_line(n_selected, n, n_correct) == want == '0.08333333333333333\t0.6833333333333333'
    assert train.metrics_line(0, 3, 3) == '0.0\t1.0'


# ---- the script itself: tests/golden/train_sampled.npz (tools/make_script_fixtures.py) ----------------------------------------
def test_hash_table_choice_and_metrics_equal_the_scripts_own(stock_weights):
    """TrainScript.load_sample_data, TrainSampledScript.choose_new_samples and write_sampling_metrics themselves, two cycles by
    hand on one script object: the hash table, the remaining failed samples, the counts and the metrics lines."""
    from conftest import golden
    from oracle import keras_gru
    from test_gpu_parity import TOL_RAW
    g = golden('train_sampled.npz')
    inputs, targets, predicted = g['inputs'], g['targets'], g['predictions']
    n = len(inputs)
    assert inputs.shape == (n, 29, 13) and targets.shape == predicted.shape == (n, 1) and predicted.dtype == np.float32 and n >= 150
    assert np.abs(predicted.astype(np.float64) - 0.5).min() > TOL_RAW
    assert np.array_equal(keras_gru.predict(inputs, stock_weights), predicted)                  # the float32 restated network's
    assert np.array_equal(inputs.astype(np.float32).astype(np.float64), inputs)                 # a float32 upload loses nothing

    hashes = train.sample_hashes(inputs, targets)
    assert hashes == [ref.calc_sample_hash(i, t) for i, t in zip(inputs, targets)]
    hash_to_ind = {h: i for i, h in enumerate(hashes)}
    table = np.array([hash_to_ind[h] for h in hashes])
    assert np.array_equal(table, g['hash_to_ind'])
    assert np.array_equal(train.eligible_mask(hashes), g['hash_to_ind'] == np.arange(n))
    # what the fixture must hold: three groups of duplicated rows with equal targets, one of them failing, and one
    # duplicated input with two targets (two hashes)
    failing = ((predicted > 0.5) != (targets > 0.5)).reshape(-1)
    groups = [np.flatnonzero(table == i) for i in np.unique(table) if np.count_nonzero(table == i) > 1]
    assert len(groups) >= 3 and any(failing[grp].all() for grp in groups)
    flat = inputs.reshape(n, -1)
    split = [(a, b) for a in range(n) for b in np.flatnonzero((flat[a + 1:] == flat[a]).all(axis=1)) + a + 1 if hashes[a] != hashes[b]]
    assert split and all(targets[a, 0] != targets[b, 0] for a, b in split)
    # the wrong reading: first duplicate wins
    first = {}
    for i, h in enumerate(hashes):
        first.setdefault(h, i)
    assert not np.array_equal(np.array([first[h] for h in hashes]), g['hash_to_ind'])

    def remaining_rows(table_of, samples):
        failed = {calc_sample_hash(inp, target) for inp, pred, target in zip(inputs, predicted, targets) if (pred > 0.5) != (target > 0.5)}
        return sorted(table_of[h] for h in failed - samples)

    samples, mutant_fails = set(), []
    n_correct = int(np.count_nonzero(~failing))
    for c in (0, 1):
        k, want = int(g['num_sample_chunk_%d' % c]), g['remaining_%d' % c].tolist()
        assert remaining_rows(hash_to_ind, samples) == want
        mutant_fails.append(remaining_rows(first, samples) != want)
        chosen = g['chosen_%d' % c].tolist()
        assert set(chosen) <= set(want) and len(chosen) == min(k, len(want)) and (k < len(want)) == (c == 0)
        samples |= {hashes[i] for i in chosen}
        assert len(samples) == int(g['n_samples_%d' % c])
        assert float(g['correct_%d' % c]) == float(n_correct / n)
        assert train.metrics_line(len(samples), n, n_correct) == str(g['line_%d' % c])
    assert not remaining_rows(hash_to_ind, samples)
    assert mutant_fails[0]              # first-duplicate-wins names other rows while the failing group still remains

    # the restated loop, one cycle: a legal outcome of the script's islice, and its line
    class Stub:
        def predict(self, x):
            return predicted

        def fit(self, *args, **kw):
            pass
    per_cycle, lines, _ = ref.run(Stub(), inputs, targets, 1, 1, 16, int(g['num_sample_chunk_0']), 'index')
    assert per_cycle[0] == g['remaining_0'][:int(g['num_sample_chunk_0'])].tolist() and lines == [str(g['line_0'])]
