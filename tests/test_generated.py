"""GPU: the generating session (csrc/generate_device.h, pe_generator) against the restatement of the script's generators and the
per-chunk public API it replaces.

Every comparison is equality: the mix kernel spells numpy's float32 / float64 operations one by one; the frames are the offline
front end's, which is what a float-mode ``Listener`` runs per chunk; the trainer sees the same float32 rows in stream order.
"""
import ctypes
import functools
import random
from types import SimpleNamespace

import numpy as np
import pytest

import generated_reference as ref
from generated_reference import B, draws, inputs, tone
from mycroft_precise_amd import params as P
from mycroft_precise_amd import synth
from mycroft_precise_amd._lib import GEN_FILE, HipEngine
from mycroft_precise_amd.generated import Generator
from mycroft_precise_amd.model import ModelParams, save_weights
from mycroft_precise_amd.network_runner import HipRunner, Listener
from mycroft_precise_amd.train import RMSPROP_EPS, RMSPROP_LR, RMSPROP_RHO, GeneratedTrainer, Trainer
from mycroft_precise_amd.vectorization import add_deltas

pytestmark = pytest.mark.gpu

INVALID = 1


@functools.lru_cache(maxsize=None)
def weights(seed=7):
    return synth.make_weights(P.pr.n_mfcc, (20,), seed=seed)


@pytest.fixture(scope='module')
def model_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('generated') / 'random20.npz')
    save_weights(path, weights())
    return path


@functools.lru_cache(maxsize=None)
def expected(C, mode):
    """the restatement's stream over the shared inputs, computed once: per file [(i, chunk, chunk_ww, targets, label)]"""
    backgrounds, positives, negatives = inputs(C)
    return ref.run(backgrounds, positives, negatives, draws(), C, B, mode=mode)[0]


def planned(C, mode, runner):
    gen = Generator(runner, *inputs(C), chunk_size=C)
    plan = gen.plan(ref.CountingRng(draws()), replay=mode)
    gen.load(plan)
    return gen, plan


def mixed_of(chunks):
    return np.concatenate([c[1] for c in chunks]) if chunks else np.zeros(0)


# ---- the mix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,mode', [(512, 'reference'), (512, 'tail'), (1000, 'reference'), (2048, 'reference'), (2048, 'tail')])
def test_mixed_audio_equals_the_restatement(C, mode):
    per_file = expected(C, mode)
    runner = HipRunner(weights=weights())
    gen, plan = planned(C, mode, runner)
    assert np.float32(plan.files['audio_volume'][0]) != plan.files['audio_volume'][0]      # u = 0.37: the float32 rounding matters
    for f, chunks in enumerate(per_file):
        want = mixed_of(chunks)
        got = gen.audio(f)
        assert got.dtype == np.float64 and got.size == want.size == len(chunks) * C
        assert got.tobytes() == want.tobytes()
        if want.size > 700:                                                                    # a range from the middle
            assert gen.audio(f, 300, 401).tobytes() == want[300:701].tobytes()
    # the same plan in passes of one file each: the same samples, the same rows
    rows = gen.vectorize(np.arange(plan.n_chunks))
    runner.engine.set_clip_pass_bytes(3 * C * 8)
    gen.load(plan)
    assert sum(1 for chunks in per_file if chunks) >= 3
    for f, chunks in enumerate(per_file):
        assert gen.audio(f).tobytes() == mixed_of(chunks).tobytes()
    assert gen.vectorize(np.arange(plan.n_chunks)).tobytes() == rows.tobytes()
    gen.close()


def test_clip_silence_clip_inside_one_chunk():
    """short gaps (a sample rate of 100: silences of 50 .. 250 samples) and short clips: chunks that switch source many times"""
    C = 512
    backgrounds = [tone(1, 6000), tone(2, 3 * C + 1)]
    positives, negatives = [tone(3, 300), tone(4, 1)], [tone(5, 170), tone(6, C - 1)]
    r = random.Random(3)
    d = [r.random() for _ in range(600)]
    per_file, _, n_draws = ref.run(backgrounds, positives, negatives, d, C, B, sample_rate=100, mode='tail')
    gen = Generator(HipRunner(weights=weights()), backgrounds, positives, negatives, chunk_size=C, sample_rate=100)
    plan = gen.plan(ref.CountingRng(d), replay='tail')
    assert plan.n_draws == n_draws
    ends = np.cumsum(plan.segments['length'][:int(plan.files['n_segments'][0])])
    inside = np.bincount(ends // C)                 # segment ends per chunk of file 0
    assert inside.max() >= 3
    gen.load(plan)
    for f, chunks in enumerate(per_file):
        assert gen.audio(f).tobytes() == mixed_of(chunks).tobytes() and len(chunks) >= 3
    gen.close()


# ---- the rows --------------------------------------------------------------------------------------------------------------
def listener_windows(lis, per_file):
    """float32 windows of a float-mode Listener cleared per file and fed every chunk; one per chunk, in global order"""
    out = []
    for chunks in per_file:
        lis.clear()
        for _, chunk, _, _, _ in chunks:
            out.append(lis.update_vectors(chunk).astype(np.float32))
            assert lis._float_mode
    return np.stack(out)


@pytest.mark.parametrize('C', [512, 1000, 2048])
def test_rows_equal_the_listener_per_chunk(model_file, C):
    per_file = expected(C, 'reference')
    runner = HipRunner(weights=weights())
    gen, plan = planned(C, 'reference', runner)
    windows = listener_windows(Listener(model_file, C), per_file)
    assert windows.shape[0] == plan.n_chunks
    want = windows[plan.ids]
    got = gen.vectorize(plan.ids)
    assert got.dtype == np.float32 and got.shape == (plan.ids.size, P.pr.n_features, P.pr.n_mfcc)
    assert got.tobytes() == want.tobytes()
    assert plan.ids[0] == 0 and got[-1].all() and not got[0][:-1].any()     # before the first frame: zero rows
    assert got[0][-1].any() == (C >= P.pr.window_samples)
    assert np.any((got == 0).all(axis=2).any(axis=1) & (got != 0).any(axis=(1, 2)))       # ... and windows that are partly zero
    order = np.random.default_rng(C).permutation(plan.n_chunks)
    ids = np.concatenate([order, order[:5], [order[0]] * 3])                # every chunk, shuffled, some twice
    assert gen.vectorize(ids).tobytes() == windows[ids].tobytes()
    if C == 2048:       # a use_delta engine: the delta columns of the same windows
        hpr = P.pr.copy()
        hpr.__dict__['use_delta'] = True
        eng = HipEngine(hpr, synth.make_weights(2 * hpr.n_mfcc, (20,), seed=3))
        gen_d = Generator(SimpleNamespace(engine=eng), *inputs(C), chunk_size=C)
        gen_d.load(gen_d.plan(ref.CountingRng(draws())))
        got_d = gen_d.vectorize(ids)
        assert got_d.shape[2] == 2 * hpr.n_mfcc
        assert got_d.tobytes() == np.stack([add_deltas(w) for w in windows[ids]]).astype(np.float32).tobytes()
        gen_d.close()
    gen.close()


def test_append_puts_rows_and_targets_behind_the_resident_set():
    C = 512
    runner = HipRunner(weights=weights())
    gen, plan = planned(C, 'reference', runner)
    rows = gen.vectorize(plan.ids)
    assert set(plan.targets.tolist()) == {0.0, 1.0}
    T, F = P.pr.n_features, P.pr.n_mfcc
    rng = np.random.default_rng(5)
    X = rng.normal(0, 1, (7, T, F)).astype(np.float32)
    y = (rng.random(7) < 0.5).astype(np.float32)
    k = plan.ids.size // 2
    for validation in (False, True):
        trainer = Trainer(weights(), ModelParams(recurrent_units=20))
        trainer.set_data(X, y, validation=validation)
        gen.append_to(trainer, plan.ids[:k], plan.targets[:k], validation=validation)
        gen.append_to(trainer, plan.ids[k:], plan.targets[k:], validation=validation)
        assert trainer.n_samples(validation) == 7 + plan.ids.size and trainer.n_samples(not validation) == 0
        feats, targets = trainer._t.get_data(validation=validation)
        assert feats[:7].tobytes() == X.tobytes() and targets[:7].tobytes() == y.tobytes()
        assert feats[7:].tobytes() == rows.tobytes()
        assert targets[7:].tobytes() == plan.targets.tobytes()
        trainer.close()
    gen.close()


# ---- fit_generator ---------------------------------------------------------------------------------------------------------
def test_generated_trainer_equals_a_trainer_stepped_over_the_same_batches():
    C, batch, epochs, steps = 2048, 8, 2, 3
    backgrounds = [tone(31, 30000), tone(32, 21000)]
    positives, negatives = [tone(33, 20000)], [tone(34, 5000)]
    T, F = P.pr.n_features, P.pr.n_mfcc
    rng = np.random.default_rng(2)
    Xv = rng.normal(0, 1, (6, T, F)).astype(np.float32)
    yv = (rng.random(6) < 0.5).astype(np.float32)

    runner = HipRunner(weights=weights())
    gen = Generator(runner, backgrounds, positives, negatives, chunk_size=C)
    trainer = Trainer(weights(), ModelParams(recurrent_units=20), seed=5)
    seen = []
    history = GeneratedTrainer(trainer, gen, files_per_plan=2).fit(epochs, steps, batch, random.Random(9), validation_data=(Xv, yv),
                                                                    callback=lambda epoch, logs: seen.append((epoch, logs['loss'])))

    # the same stream, drawn the same way, as host arrays
    other_gen = Generator(runner, backgrounds, positives, negatives, chunk_size=C)
    r = random.Random(9)
    X, y, per_plan, first_file = [], [], [], []
    while sum(per_plan) < epochs * steps * batch:
        plan = other_gen.plan(r, files=[0, 1])
        other_gen.load(plan)
        X.append(other_gen.vectorize(plan.ids))
        y.append(plan.targets)
        per_plan.append(plan.ids.size)
        first_file.append(int(np.count_nonzero(plan.ids < plan.chunk_offsets[1])))
    print('samples per plan', per_plan, 'of them in the first file', first_file)
    assert len(per_plan) >= 2 and per_plan[0] % batch and first_file[0] % batch and 0 < first_file[0] < per_plan[0]
    X, y = np.concatenate(X), np.concatenate(y)
    assert y.sum() >= 2 and 0 in per_plan                           # wake words among the samples; a plan that brought none
    assert trainer.n_samples() == X.shape[0]                        # planned only as far as the batches needed
    other = Trainer(weights(), ModelParams(recurrent_units=20), seed=5)
    other.set_data(X, y)
    p = other.params
    losses = [other._t.step(np.arange(s * batch, (s + 1) * batch), dropout_rate=p.dropout, seed=other.seed, step=s, loss_bias=p.loss_bias,
                            lr=RMSPROP_LR, rho=RMSPROP_RHO, eps=RMSPROP_EPS, frozen_mask=other.frozen_mask) for s in range(epochs * steps)]
    assert history['loss'] == [float(np.mean(losses[e * steps:(e + 1) * steps])) for e in range(epochs)]
    assert seen == list(enumerate(history['loss']))
    assert trainer._t.get_weights().tobytes() == other._t.get_weights().tobytes()
    assert trainer._t.get_accumulators().tobytes() == other._t.get_accumulators().tobytes()
    assert trainer._step == epochs * steps
    other.set_data(Xv, yv, validation=True)
    assert (history['val_loss'][-1], history['val_acc'][-1]) == other._evaluate_resident('validation')
    assert np.any(trainer._t.get_weights() != Trainer(weights(), ModelParams(recurrent_units=20), seed=5)._t.get_weights())
    gen.close(); other_gen.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_the_library_checks_its_arguments_itself():
    C = 512
    eng = HipEngine(P.pr, weights())
    gen, plan = planned(C, 'reference', SimpleNamespace(engine=eng))
    session = gen._session()
    lib, h = session._lib, session._h
    err = lambda: lib.pe_last_error(eng._h)
    ids = plan.ids.astype(np.int32)
    rows = gen.vectorize(ids)
    usable = lambda: gen.vectorize(ids).tobytes() == rows.tobytes()

    # a plan whose segments do not fill a file, or overrun it, or leave their clip: refused, and the resident plan stays
    files = np.ascontiguousarray(plan.files, dtype=GEN_FILE)
    set_plan = lambda segments: lib.pe_generator_set_plan(h, files.ctypes.data, files.size, segments.ctypes.data, segments.size)
    last_of_file0 = int(files['n_segments'][0]) - 1
    for field, delta, word in (('length', -1, b'file 0'), ('length', 1, b'file 0'), ('clip', 100, b'segment %d' % last_of_file0)):
        bad = plan.segments.copy()
        bad[field][last_of_file0] += delta
        assert set_plan(bad) == INVALID and word in err(), err()
        assert usable()
    bad = plan.segments.copy()
    s = int(np.flatnonzero(bad['clip'] >= 0)[0])
    bad['first'][s] += len(gen.clips[int(bad['clip'][s])])
    assert set_plan(bad) == INVALID and b'segment %d' % s in err() and usable()
    bad_files = files.copy()
    bad_files['background'][1] = len(gen.backgrounds)
    assert lib.pe_generator_set_plan(h, bad_files.ctypes.data, files.size, plan.segments.ctypes.data, plan.segments.size) == INVALID
    assert b'file 1' in err() and usable()

    # an id outside the plan
    out = np.full((2, P.pr.n_features, P.pr.n_mfcc), 7.0, np.float32)
    for pair in ([0, plan.n_chunks], [-1, 0]):
        two = np.array(pair, np.int32)
        assert lib.pe_generator_vectorize(h, two.ctypes.data, 2, out.ctypes.data) == INVALID
        assert b'outside' in err() and b'ids[%d]' % (1 if pair[0] == 0 else 0) in err() and np.all(out == 7.0)
    with pytest.raises(ValueError):
        gen.vectorize([plan.n_chunks])
    assert lib.pe_generator_audio(h, len(gen.backgrounds), 0, 1, out.ctypes.data) == INVALID and b'file' in err()

    # a trainer of another shape, a target of 2.0
    two = np.array([0, 1], np.int32)
    y = np.array([0.0, 2.0], np.float32)
    other = Trainer(synth.make_weights(P.pr.n_mfcc + 1, (20,), seed=3), ModelParams(recurrent_units=20))
    assert lib.pe_generator_append(h, other._t._h, 1, two.ctypes.data, np.zeros(2, np.float32).ctypes.data, 2) == INVALID
    assert b'trainer takes' in err() and other.n_samples() == 0
    with pytest.raises(ValueError):
        gen.append_to(other, [0, 1], [0.0, 1.0])
    trainer = Trainer(weights(), ModelParams(recurrent_units=20))
    assert lib.pe_generator_append(h, trainer._t._h, 1, two.ctypes.data, y.ctypes.data, 2) == INVALID
    assert b'targets[1]' in err() and b'2' in err() and trainer.n_samples() == 0
    assert lib.pe_generator_append(h, trainer._t._h, 0, two.ctypes.data, np.zeros(2, np.float32).ctypes.data, 2) == INVALID      # source
    assert lib.pe_generator_append(h, None, 1, two.ctypes.data, y.ctypes.data, 2) == INVALID
    assert usable()
    gen.append_to(trainer, [0, 1], [0.0, 1.0])
    assert trainer.n_samples() == 2

    # offsets as pe_miner_create checks them
    g2 = ctypes.c_void_p()
    audio = np.zeros(10, np.float32)
    good, down = np.array([0, 10], np.int64), np.array([0, 10, 5], np.int64)
    create = lambda bo, co, chunk: lib.pe_generator_create(eng._h, audio.ctypes.data, bo.ctypes.data, bo.size - 1, audio.ctypes.data,
                                                            co.ctypes.data, co.size - 1, chunk, ctypes.byref(g2))
    assert create(down, good, 4) == INVALID and b'background 1' in err() and not g2.value
    assert create(good, down, 4) == INVALID and b'clip 1' in err()
    assert create(good, good, 0) == INVALID and create(np.array([1, 10], np.int64), good, 4) == INVALID
    # an engine that is closed takes its sessions with it; the session then refuses by name
    eng.close()
    with pytest.raises(ValueError):
        gen.vectorize([0])


# ---- the script itself: tests/golden/train_generated.npz (tools/make_script_fixtures.py) --------------------------------------
@pytest.mark.parametrize('C', [512, 2048])
def test_generator_equals_the_scripts_own_stream(model_file, C):
    """TrainGeneratedScript.vectors_from_fn's own output over five background files: the planner replays its draws, the mix
    gives its merged chunks bit for bit, the ids and targets are its labels, and the rows are its windows within TOL_FEAT32 --
    what tests/test_gpu_parity.py asks of float32 ring rows against the reference's Listener -- and, bit for bit as in
    test_rows_equal_the_listener_per_chunk, the project's Listener fed the same chunks."""
    from conftest import golden
    from test_gpu_parity import TOL_FEAT32
    g = golden('train_generated.npz')
    k = '_%d' % C
    backgrounds, positives, negatives, fixture_draws = ref.fixture_pools(g, C)
    labels, offsets, audio_ids = g['label' + k], g['chunk_offsets' + k], g['audio_ids' + k]
    runner = HipRunner(weights=weights())
    gen = Generator(runner, backgrounds, positives, negatives, chunk_size=C, buffer_samples=int(g['buffer_samples']))
    plan = gen.plan(ref.CountingRng(fixture_draws))
    assert plan.n_draws == int(g['file_draws' + k].sum()) and plan.chunk_offsets.tolist() == offsets.tolist()
    assert plan.ids.tolist() == np.flatnonzero(labels >= 0).tolist() and plan.targets.tolist() == labels[labels >= 0].tolist()
    assert set(plan.targets.tolist()) == {0.0, 1.0} and plan.ids.size < plan.n_chunks
    gen.load(plan)
    mixed = [gen.audio(f) for f in range(len(backgrounds))]
    file_of = np.searchsorted(offsets, audio_ids, side='right') - 1
    assert set(file_of.tolist()) == set(range(len(backgrounds)))
    for n, (f, chunk) in enumerate(zip(file_of.tolist(), audio_ids.tolist())):
        i = chunk - int(offsets[f])
        got = mixed[f][i * C:(i + 1) * C]
        assert got.dtype == np.float64 and got.tobytes() == g['audio' + k][n * C:(n + 1) * C].tobytes(), (f, i)
    rows = gen.vectorize(plan.ids)
    want = g['windows' + k]
    assert rows.dtype == np.float32 and rows.shape == want.shape
    worst = float(np.abs(rows.astype(np.float64) - want).max())
    print('C=%d: %d rows, worst |row - the script\'s window| %.3g (bound %.3g)' % (C, len(rows), worst, TOL_FEAT32))
    assert worst <= TOL_FEAT32
    lis = Listener(model_file, C)
    windows = []
    for audio in mixed:
        lis.clear()
        for i in range(audio.size // C):
            windows.append(lis.update_vectors(audio[i * C:(i + 1) * C]).astype(np.float32))
    assert rows.tobytes() == np.stack(windows)[plan.ids].tobytes()
    gen.close()
