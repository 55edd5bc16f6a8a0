"""GPU: what the three data sessions (pe_miner, pe_generator, pe_augmenter) share on the host side of the engine.

A closed session gives back every byte it took: ``pe_info.device_bytes`` counts a session's buffers with its engine's, so a
buffer a session declares but does not release shows as a difference between two rounds of the same work.  The three append
entry points refuse a wrong trainer, source, target or id with the same words; the expected texts below were printed by the
library as it stood before these checks were stated once, and are kept as literals.
"""
import numpy as np
import pytest

from mycroft_precise_amd import _lib
from mycroft_precise_amd import params as P
from mycroft_precise_amd import synth
from mycroft_precise_amd._lib import AUG_COPY, AUG_PIECE, GEN_FILE, GEN_SEGMENT, HipAugmenter, HipEngine, HipGenerator, HipMiner, HipTrainer
from mycroft_precise_amd.threshold_decoder import ThresholdDecoder

pytestmark = pytest.mark.gpu

C = 2048
T = P.pr.n_features


def tone(seed, n):
    """load_audio's output for a synthetic wav: k / 32767 in float32"""
    return synth.stream_pcm(seed, n).astype(np.float32) / np.float32(32767.0)


def delta_params():
    hpr = P.pr.copy()
    hpr.__dict__['use_delta'] = True
    return hpr


def delta_weights():
    return synth.make_weights(2 * P.pr.n_mfcc, (20,), seed=3)


@pytest.fixture(scope='module')
def engines(stock_weights):
    """name -> (engine, weights of a trainer that fits it); every engine decodes, so that a scan allocates `conf`"""
    made = {'stock': (HipEngine(P.pr, stock_weights), stock_weights),
            'use_delta': (HipEngine(delta_params(), delta_weights()), delta_weights()),
            'two_models': (HipEngine(P.pr, [stock_weights, stock_weights]), stock_weights)}
    for engine, _ in made.values():
        engine.set_decoder(ThresholdDecoder(P.pr.threshold_config, P.pr.threshold_center))
    yield made
    for engine, _ in made.values():
        engine.close()


def trainer_for(engine, weights):
    return HipTrainer(weights, T, engine.feature_size)


# ---- one session of each kind over the smallest inputs that make every buffer it grows on demand exist ----------------------
def open_miner(engine):
    return HipMiner(engine, [tone(1, 3 * C + 1), tone(2, 3 * C + 1)], C, P.pr.buffer_samples)


def use_miner(miner, trainer):
    n = miner.n_chunks
    assert n == 6
    hits, _, scores = miner.scan(threshold=-1.0, capacity=n, return_scores=True)
    assert hits.tolist() == list(range(n)) and scores.size == n
    if miner.engine.n_models > 1:
        miner.scan(threshold=-1.0, capacity=n, model=1)
    assert miner.vectorize(hits).shape == (n, T, P.pr.n_mfcc)
    miner.append(trainer, hits)
    return n


def open_generator(engine):
    gen = HipGenerator(engine, [tone(3, 2 * C + 1), tone(4, 2 * C + 1)], [tone(5, 700)], C)
    files = np.zeros(2, dtype=GEN_FILE)
    segments = np.zeros(4, dtype=GEN_SEGMENT)
    files['background'] = [0, 1]
    files['audio_volume'], files['rms'] = 0.5, 0.1
    files['first_segment'], files['n_segments'] = [0, 3], [3, 1]
    segments['clip'] = [-1, 0, -1, -1]                      # file 0: background, the clip over it, background; file 1: background
    segments['first'] = [0, 100, 0, 0]
    segments['length'] = [1000, 500, 2 * C - 1500, 2 * C]
    segments['volume'], segments['rms'] = 1.0, 0.2
    gen.set_plan(files, segments)
    return gen


def use_generator(gen, trainer):
    n = gen.n_chunks
    assert n == 4
    assert gen.audio(0).size == 2 * C
    ids = np.arange(n)
    assert gen.vectorize(ids).shape == (n, T, gen.engine.feature_size)
    gen.append(trainer, ids, np.array([0, 1, 0.25, 1], dtype=np.float32))
    return n


CLIP_LENGTHS = (1700, 2401, 3000)


def open_augmenter(engine):
    aug = HipAugmenter(engine, [tone(6 + i, n) for i, n in enumerate(CLIP_LENGTHS)], [tone(10, 2000), tone(11, 4000)])
    copies = np.zeros(3, dtype=AUG_COPY)
    pieces = np.zeros(4, dtype=AUG_PIECE)
    copies['clip'], copies['ratio'] = [0, 1, 2], 0.25
    copies['first_piece'], copies['n_pieces'] = [0, 1, 2], [1, 1, 2]
    pieces['noise'] = [0, 1, 1, 0]                          # the last copy takes its noise from both recordings
    pieces['first'] = [100, 0, 500, 0]
    pieces['length'] = [1700, 2401, 2000, 1000]
    aug.set_plan(copies, pieces)
    return aug


def use_augmenter(aug, trainer):
    n = aug.n_copies
    assert n == 3
    assert aug.volumes(overflowed=True)[2].size == n
    assert aug.audio(2).size == aug.pcm(2).size == CLIP_LENGTHS[2]
    assert aug.vectorize().shape == (n, T, aug.engine.feature_size)
    aug.append(trainer, None, np.array([0, 1, 0.5], dtype=np.float32))
    return n


SESSIONS = {'miner': (open_miner, use_miner), 'generator': (open_generator, use_generator), 'augmenter': (open_augmenter, use_augmenter)}
CASES = [(kind, name) for kind in sorted(SESSIONS) for name in ('stock', 'use_delta')] + [('miner', 'two_models')]


@pytest.mark.parametrize('kind,name', CASES)
def test_a_closed_session_gives_its_memory_back(engines, kind, name):
    """two rounds on one engine: the first lets the engine's own staging buffers reach their size"""
    engine, weights = engines[name]
    open_session, use = SESSIONS[kind]
    after_close, while_open = [], []
    for _ in range(2):
        trainer = trainer_for(engine, weights)
        session = open_session(engine)
        n = use(session, trainer)
        assert trainer.n_samples() == n
        while_open.append(int(engine.info().device_bytes))
        session.close()
        trainer.close()
        after_close.append(int(engine.info().device_bytes))
    print('%s on %s: device_bytes open %r, closed %r' % (kind, name, while_open, after_close))
    assert after_close[1] == after_close[0]
    assert while_open[1] > after_close[1]


# ---- the three appends refuse alike ---------------------------------------------------------------------------------------
def append_of(kind, lib, session):
    """-> f(trainer handle, source, id, target) of the session's append entry point over one id and one target"""
    def call(trainer, source, i, y):
        ids, targets = np.array([i], np.int32), np.array([y], np.float32)       # alive until the call is back
        if kind == 'miner':
            return lib.pe_miner_append(session._h, trainer, source, ids.ctypes.data, 1, y)
        if kind == 'generator':
            return lib.pe_generator_append(session._h, trainer, source, ids.ctypes.data, targets.ctypes.data, 1)
        return lib.pe_augmenter_append(session._h, trainer, source, ids.ctypes.data, targets.ctypes.data, 1, 0)
    return call


SHARED_REFUSALS = {
    'other_shape': "%s: the trainer takes [29][26] inputs, the engine's windows are [29][13]",
    'source_0': '%s: source = 0',
    'null_trainer': 'null argument to %s',
}
OWN_REFUSALS = {
    'miner': {'target': 'pe_miner_append: target 1.5 is outside [0, 1]',
              'id': "pe_miner_append: hits[0] = 6 is outside the session's 6 chunks"},
    'generator': {'target': 'pe_generator_append: targets[0] = 1.5 is outside [0, 1]',
                  'id': "pe_generator_append: ids[0] = 4 is outside the plan's 4 chunks"},
    'augmenter': {'target': 'pe_augmenter_append: targets[0] = 1.5 is outside [0, 1]',
                  'id': "pe_augmenter_append: ids[0] = 3 is outside the plan's 3 copies"},
}


@pytest.mark.parametrize('kind', sorted(SESSIONS))
def test_the_appends_refuse_alike(engines, kind):
    engine, weights = engines['stock']
    lib = _lib.load()
    who = 'pe_%s_append' % kind
    session = SESSIONS[kind][0](engine)
    n = session.n_copies if kind == 'augmenter' else session.n_chunks
    fits, other = trainer_for(engine, weights), HipTrainer(delta_weights(), T, 2 * P.pr.n_mfcc)
    append = append_of(kind, lib, session)
    data = _lib.TRAIN_SOURCE_DATA
    calls = [(SHARED_REFUSALS['other_shape'] % who, lambda: append(other._h, data, 0, 0.5)),
             (SHARED_REFUSALS['source_0'] % who, lambda: append(fits._h, 0, 0, 0.5)),
             (SHARED_REFUSALS['null_trainer'] % who, lambda: append(None, data, 0, 0.5)),
             (OWN_REFUSALS[kind]['target'], lambda: append(fits._h, data, 0, 1.5)),
             (OWN_REFUSALS[kind]['id'], lambda: append(fits._h, data, n, 0.5))]
    for want, call in calls:
        rc = call()
        said = lib.pe_last_error(engine._h).decode()
        print('%d %r' % (rc, said))
        assert rc == _lib.PE_ERR_INVALID and said == want
        assert fits.n_samples() == fits.n_samples(validation=True) == other.n_samples() == other.n_samples(validation=True) == 0
    assert append(fits._h, data, n - 1, 0.5) == _lib.PE_OK and fits.n_samples() == 1       # ... and nothing else was wrong
    session.close()
    fits.close()
    other.close()
