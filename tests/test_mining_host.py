"""No GPU: the mining session's ABI surface, its chunk arithmetic, and the policy of ``IncrementalTrainer`` against the numpy
restatement of scripts/train_incremental.py:113-137 (incremental_reference.py)."""
import os
import re

import numpy as np
import pytest

import incremental_reference as ref
from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.train import IncrementalTrainer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['pe_set_weights', 'pe_trainer_append', 'pe_trainer_get_data', 'pe_miner_create', 'pe_miner_destroy', 'pe_miner_layout',
               'pe_miner_scan', 'pe_miner_vectorize', 'pe_miner_append']


def test_symbols_declared_and_bound():
    header = open(os.path.join(REPO, 'include', 'precise_engine.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.EXPORTS, name
    assert '#define PE_ABI_VERSION 8' in header and _lib.ABI_VERSION == 8


@pytest.mark.parametrize('C', [512, 2048])
def test_chunk_offsets_follow_chunk_audio(C):
    lengths = [0, 1, C - 1, C, C + 1, 2 * C, 2 * C + 1]
    counts = [len(list(ref.chunks(np.zeros(n), C))) for n in lengths]
    assert counts == [0, 0, 0, 0, 1, 1, 2]
    assert ref.chunk_offsets(lengths, C).tolist() == np.concatenate(([0], np.cumsum(counts))).tolist()
    # (pe_miner_layout itself is held to ref.chunk_offsets on the same lengths in tests/test_mining.py: it needs an engine)


@pytest.mark.parametrize('C', [1, 7, 100])
def test_locate_skips_recordings_without_a_chunk(C):
    """Miner.locate is host arithmetic over chunk_offsets: a recording without a chunk repeats its neighbour's entry, at the
    head, in the middle and at the tail of the table, and is never the answer"""
    from types import SimpleNamespace
    from mycroft_precise_amd.mining import Miner
    lengths = [0, 1, C, 0, 3 * C + 1, 1, 0, 0, C, 1, C + 1, 2 * C, 2 * C + 1, 0, 0, 0, 0, 0, 5 * C + 1, C, 0, 1]
    want = ref.locate(lengths, C)
    offsets = ref.chunk_offsets(lengths, C)
    assert len(want) == offsets[-1] == 3 + 1 + 1 + 2 + 5 and offsets[0] == offsets[4] == 0 and offsets[-1] == offsets[-4]
    session = SimpleNamespace(chunk_offsets=offsets)
    ids = np.arange(len(want))
    for order in (ids, ids[::-1], np.array([4, 4, 0, 11])):
        rec, chunk = Miner.locate(session, order)
        assert rec.dtype == chunk.dtype == np.int64
        assert list(zip(rec.tolist(), chunk.tolist())) == [want[i] for i in order]
        assert all(ref.n_chunks(lengths[r], C) > i for r, i in zip(rec.tolist(), chunk.tolist()))
    rec, chunk = Miner.locate(session, [])
    assert rec.size == chunk.size == 0


def test_round_trip_is_not_the_identity():
    """load_audio output is k / 32767 in float32; times 32767.0 that lands below k for many k and truncates to k - 1: a ring
    kernel that skipped the round trip would produce other samples."""
    audio = synth.stream_pcm(3, 16000).astype(np.float32) / np.float32(32767.0)
    back = ref.round_trip(audio.astype(np.float64))
    assert back.dtype == np.float32
    changed = np.count_nonzero(back != audio)
    assert 0 < changed < audio.size
    one = np.float32(1.0) / np.float32(32767.0)
    assert ref.round_trip(np.array([float(one)]))[0] == 0.0


# ---- the policy, with everything that touches a device replaced ------------------------------------------------------------
def fake_score(g, n_retrains):
    """a prediction in [0, 1) that depends on (global chunk id, retrains so far) alone"""
    return ((int(g) * 2654435761 + int(n_retrains) * 40503 + 12345) % 1000) / 1000.0


class FakeRunner:
    def __init__(self):
        self.n_retrains = 0

    def set_weights(self, weights):
        self.n_retrains = weights


class FakeTrainer:
    def __init__(self):
        self.fits, self.appended = 0, {False: [], True: []}

    def fit_resident(self, batch_size, epochs, shuffle=True):
        self.fits += 1
        self.snapshots = getattr(self, 'snapshots', []) + [(list(self.appended[False]), list(self.appended[True]))]

    @property
    def weights(self):
        return self.fits


class FakeMiner:
    scans = 0

    def __init__(self, runner, audios, chunk_size=2048, carry_audio=True):
        self.runner = runner
        self.chunk_offsets = ref.chunk_offsets([len(a) for a in audios], chunk_size)
        self.n_chunks = int(self.chunk_offsets[-1])

    def scan(self, first=0, threshold=0.5, capacity=None, return_scores=False):
        FakeMiner.scans += 1
        scores = np.array([fake_score(g, self.runner.n_retrains) for g in range(first, self.n_chunks)])
        hits = first + np.flatnonzero(scores > threshold)
        return hits[:capacity].astype(np.int32), int(hits.size), None

    def locate(self, hits):
        hits = np.asarray(hits, dtype=np.int64)
        rec = np.searchsorted(self.chunk_offsets, hits, side='right') - 1
        return rec, hits - self.chunk_offsets[rec]

    def append_to(self, trainer, hits, validation=False):
        trainer.appended[bool(validation)] += [int(h) for h in hits]

    def close(self):
        pass


LENGTHS = [5 * 100 + 1, 0, 12 * 100 + 7, 100, 30 * 100 + 1, 9 * 100 + 50, 17 * 100 + 1, 1, 25 * 100 + 3]
CASES = {
    # a test recording (index 4, 30 chunks) pushes the count far past delay_samples; the retrain comes at the next training chunk
    'test_recording_pushes_past': dict(flags=[0, 0, 0, 0, 1, 0, 0, 1, 0], delay=4, epochs=1, capacity=4096, threshold=0.7),
    'epochs_zero': dict(flags=[0, 0, 1, 0, 0, 0, 1, 0, 0], delay=3, epochs=0, capacity=4096, threshold=0.6),
    'capacity_below_a_cut': dict(flags=[0, 0, 0, 0, 1, 0, 0, 0, 0], delay=7, epochs=2, capacity=2, threshold=0.5),
    'capacity_one': dict(flags=[1, 0, 0, 0, 0, 0, 1, 0, 0], delay=3, epochs=1, capacity=1, threshold=0.8),
    'all_training': dict(flags=[0] * 9, delay=1, epochs=1, capacity=4096, threshold=0.9),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_incremental_policy_equals_the_scripts_loop(case):
    c = CASES[case]
    C = 100
    audios = [np.zeros(n, np.float32) for n in LENGTHS]
    offsets = ref.chunk_offsets(LENGTHS, C)
    runner, trainer = FakeRunner(), FakeTrainer()
    inc = IncrementalTrainer(trainer, runner, delay_samples=c['delay'], epochs=c['epochs'], threshold=c['threshold'], chunk_size=C,
                             capacity=c['capacity'], miner_cls=FakeMiner)
    got_hits, got_retrains = inc.run(audios, test_flags=c['flags'])

    state = {'retrains': 0, 'snapshots': []}

    def retrain(saved):
        state['retrains'] += 1
        state['snapshots'].append(len(saved))

    hits, retrains, saved, count = ref.policy_loop(
        audios, c['flags'], C, 300, c['delay'], c['epochs'], c['threshold'], lambda r: None,
        lambda r, i, chunk: fake_score(offsets[r] + i, state['retrains']), retrain)
    assert len(hits) > 3
    assert got_hits == hits
    assert got_retrains == retrains
    assert trainer.fits == len(retrains) and runner.n_retrains == len(retrains)
    assert inc.samples_since_train == count
    # routing: training hits in the training set, test hits in the validation set, each in the script's order ...
    for test in (False, True):
        assert trainer.appended[test] == [int(offsets[r] + i) for r, i, t in hits if t == test]
    # ... and at every retrain exactly the samples the script had saved by then
    assert [len(a) + len(b) for a, b in getattr(trainer, 'snapshots', [])] == state['snapshots']
    if case == 'test_recording_pushes_past':
        first_after = (5, 0)            # the first chunk of the first training recording behind the test recording
        assert first_after in retrains
        in_test = sum(1 for r, i, t in hits if r == 4)
        assert in_test > c['delay']
    if case == 'epochs_zero':
        assert retrains == [] and trainer.fits == 0
    if case.startswith('capacity'):
        assert len(retrains) >= 1


# ---- the script itself: tests/golden/train_incremental.npz (tools/make_script_fixtures.py) ------------------------------------
class TableMiner(FakeMiner):
    """a miner that scores every chunk with the fixture's confidence, whatever was retrained"""
    conf = None

    def scan(self, first=0, threshold=0.5, capacity=None, return_scores=False):
        hits = first + np.flatnonzero(self.conf[first:] > threshold)
        return hits[:capacity].astype(np.int32), int(hits.size), None


def test_restatement_and_policy_equal_the_scripts_own_run(stock_weights):
    """TrainIncrementalScript.train_on_audio itself over four recordings on one script object (retrain replaced by a recorder, so
    every chunk is judged by the stock network): confidences, hits, saved int16 rings, retrain points."""
    from conftest import golden
    from oracle import listener as ol
    from test_gpu_parity import TOL_DECODE
    g = golden('train_incremental.npz')
    audios = ref.fixture_recordings(g)
    C, B, delay, epochs = (int(g[n]) for n in ('chunk_size', 'buffer_samples', 'delay_samples', 'epochs'))
    threshold = float(g['threshold'])
    flags = (g['flag_draws'] > 0.8).tolist()
    hits = [tuple(h) for h in g['hits'].tolist()]
    # what the fixture must hold to pin anything
    assert len(audios) >= 3 and sum(flags) == 1 and len(hits) >= 6 and g['saved'].shape == (len(hits), B) and g['saved'].dtype == np.int16
    assert any(r == 1 and (i + 1) * C < B for r, i, _ in hits)                      # a ring that still holds the first recording's tail
    assert np.abs(g['conf'] - threshold).min() > TOL_DECODE
    assert len(g['retrains']) >= 1 and g['chunk_starts'].tolist() == ref.chunk_offsets([len(a) for a in audios], C).tolist()

    lis = ol.OracleListener(stock_weights)
    raws, confs = [], []

    def predict(r, i, chunk):
        raws.append(lis.update_raw32(chunk))
        confs.append(lis.threshold_decoder.decode(raws[-1]))
        return confs[-1]

    record = []
    got_hits, got_retrains, saved, count = ref.policy_loop(audios, flags, C, B, delay, epochs, threshold, lambda r: lis.clear(), predict,
                                                           lambda saved: record.append(len(saved)))
    assert np.array_equal(np.array(raws, dtype=np.float32), g['raw']) and np.array_equal(np.array(confs), g['conf'])      # (as test_oracle.py)
    assert [(r, i, int(t)) for r, i, t in got_hits] == hits
    assert [(r, i, n) for (r, i), n in zip(got_retrains, record)] == [tuple(x) for x in g['retrains'].tolist()]
    assert count == int(g['samples_since_train'])
    # a retrain withheld by the test flag: the count stood at delay_samples or above inside the test recording
    r_test = flags.index(True)
    in_test = [n for n, (r, i, t) in enumerate(hits) if r == r_test]
    before = max([n for r, i, n in g['retrains'].tolist() if r < r_test], default=0)
    assert in_test and in_test[-1] + 1 - before >= delay and not any(r == r_test for r, _, _ in g['retrains'].tolist())

    offsets = g['chunk_starts']
    ids = [int(offsets[r] + i) for r, i, _ in hits]
    rings = ref.rings(audios, C, B, only=set(ids))
    assert np.array_equal(np.array([ref.saved_pcm(rings[i]) for i in ids]), g['saved'])
    for (ring, test), want in zip(saved, g['saved']):
        assert np.array_equal(ring, want.astype(np.float32) / np.float32(32767.0))
    # the wrong reading: a ring cleared per recording fails against the fixture, at the early hit of the second recording
    cleared = ref.rings(audios, C, B, carry_audio=False, only=set(ids))
    wrong = [n for n, i in enumerate(ids) if not np.array_equal(ref.saved_pcm(cleared[i]), g['saved'][n])]
    assert wrong and all(hits[n][0] >= 1 and (hits[n][1] + 1) * C < B for n in wrong), wrong

    # IncrementalTrainer over the fixture's confidences retrains where the script did
    runner, trainer = FakeRunner(), FakeTrainer()
    TableMiner.conf = g['conf']
    inc = IncrementalTrainer(trainer, runner, delay_samples=delay, epochs=epochs, threshold=threshold, chunk_size=C, miner_cls=TableMiner)
    inc_hits, inc_retrains = inc.run(audios, test_flags=flags)
    assert [(r, i, int(t)) for r, i, t in inc_hits] == hits and inc_retrains == got_retrains and inc.samples_since_train == count
    assert [len(a) + len(b) for a, b in trainer.snapshots] == record
