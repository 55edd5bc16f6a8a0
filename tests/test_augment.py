"""GPU: the augmenting session (csrc/augment_device.h, pe_augmenter) against the restatement of precise-add-noise, the fixture the
reference's own code wrote, and the per-copy public API it replaces.

Every comparison is equality of bytes: the two energy sums are the sequential chains Python's sum() runs, the mix kernel spells
numpy's float32 / float64 operations one by one, and the rows are pe_vectorize_clips' launch over the reloaded copies.
"""
import functools
import random
import wave
from types import SimpleNamespace

import numpy as np
import pytest

import augment_reference as ref
from conftest import golden
from mycroft_precise_amd import params as P
from mycroft_precise_amd import synth
from mycroft_precise_amd import vectorization
from mycroft_precise_amd._lib import HipEngine
from mycroft_precise_amd.augment import NoiseAugmenter
from mycroft_precise_amd.model import ModelParams
from mycroft_precise_amd.network_runner import HipRunner
from mycroft_precise_amd.train import Trainer
from mycroft_precise_amd.vectorization import add_deltas
from test_augment_host import fixture_pools, pools, tone

pytestmark = pytest.mark.gpu

CLIP_LENGTHS = (1, 65, 1599, 1600, 2401, 24000, 26000)      # below / at / above one window; a whole buffer; one that is cropped
NOISE_LENGTHS = (1, 300, 700, 1000)
INFLATION = 3
SEED = 13


@functools.lru_cache(maxsize=None)
def weights(seed=7):
    return synth.make_weights(P.pr.n_mfcc, (20,), seed=seed)


@functools.lru_cache(maxsize=None)
def expected():
    """the shared inputs and the restatement's copies over them, computed once"""
    clips, noises = pools(CLIP_LENGTHS, NOISE_LENGTHS)
    copies = ref.run(clips, ref.Pool(noises), random.Random(SEED), INFLATION)
    assert all(np.isfinite(c.noise_volume) and c.noise_volume > 0 and ref.out_of_range(c.mix) == 0 for c in copies)
    return clips, noises, copies


@functools.lru_cache(maxsize=None)
def expected_rows():
    """vectorize() of every reloaded copy, one call per copy as a user of the reference's scripts would: float32 [n, T, n_mfcc]"""
    assert P.pr.max_samples == 24000
    return np.stack([vectorization.vectorize(ref.loaded(ref.saved(c.mix))) for c in expected()[2]]).astype(np.float32)


def planned(runner, labels=None):
    clips, noises, copies = expected()
    aug = NoiseAugmenter(runner, clips, noises, labels)
    plan = aug.plan(random.Random(SEED), INFLATION)
    aug.load(plan)
    assert plan.n_copies == len(copies) == 21
    return aug, plan


def test_volumes_equal_the_restatement():
    clips, noises, copies = expected()
    aug, plan = planned(HipRunner(weights=weights()))
    va, vn, overflowed = aug.volumes()
    assert va.dtype == vn.dtype == np.float64 and overflowed.dtype == np.int64
    assert va.tobytes() == np.array([copies[c * INFLATION].clip_volume for c in range(len(clips))]).tobytes()
    assert vn.tobytes() == np.array([c.noise_volume for c in copies]).tobytes()
    assert overflowed.tolist() == [0] * len(copies)
    # neither sum is a tree: numpy's pairwise float32 sum of the long clip is another number
    assert va[5] != float(np.sqrt(np.float64(np.sum(clips[5] ** 2))))
    aug.close()


def test_audio_and_pcm_equal_the_restatement():
    clips, noises, copies = expected()
    aug, plan = planned(HipRunner(weights=weights()))
    assert plan.copies['n_pieces'].max() >= 40 and plan.copies['n_pieces'].min() == 1
    for o, c in enumerate(copies):
        mixed, saved = aug.audio(o), aug.pcm(o)
        assert mixed.dtype == np.float64 and saved.dtype == np.int16 and mixed.size == saved.size == len(clips[c.clip])
        assert mixed.tobytes() == c.mix.tobytes(), o
        assert saved.tobytes() == ref.saved(c.mix).tobytes(), o
    with pytest.raises(ValueError):
        aug.audio(len(copies))
    aug.close()


def test_audio_and_pcm_equal_the_reference():
    """the fixture: what the reference's own NoiseData and save_audio computed"""
    g = golden('add_noise.npz')
    clips, noises = fixture_pools(g)
    aug = NoiseAugmenter(HipRunner(weights=weights()), clips, noises)
    plan = aug.plan(random.Random(int(g['seed'])), int(g['inflation_factor']))
    aug.load(plan)
    assert list(plan.cursor) == g['cursor'][-1].tolist() and plan.copies['ratio'].tobytes() == g['ratio'].tobytes()
    assert np.concatenate([aug.audio(o) for o in range(plan.n_copies)]).tobytes() == g['mixed'].tobytes()
    assert np.concatenate([aug.pcm(o) for o in range(plan.n_copies)]).tobytes() == g['saved'].tobytes()
    assert aug.volumes()[2].tolist() == [0] * plan.n_copies
    aug.close()


def test_vectorize_equals_vectorize_of_the_reloaded_copy():
    want = expected_rows()
    runner = HipRunner(weights=weights())
    aug, plan = planned(runner)
    got = aug.vectorize()
    assert got.dtype == np.float32 and got.shape == (plan.n_copies, P.pr.n_features, P.pr.n_mfcc)
    assert got.tobytes() == want.tobytes()
    assert not got[:9].any() and got[9:].any(axis=(1, 2)).all()         # 1, 65 and 1599 samples hold no frame ...
    assert got[9][-1].any() and not got[9][:-1].any()                   # ... 1600 exactly one
    # the cropped clip is not the uncropped one
    uncropped = aug._session().vectorize([18], max_samples=0)
    assert uncropped.tobytes() != got[18:19].tobytes()
    order = np.random.default_rng(4).permutation(plan.n_copies)
    ids = np.concatenate([order, order[:5], [order[0]] * 3])            # every copy, shuffled, some twice
    assert aug.vectorize(ids).tobytes() == want[ids].tobytes()
    # in passes of about one long copy each: the same bytes, rows, samples and counts
    runner.engine.set_clip_pass_bytes(30000 * 4)
    aug.load(plan)
    assert aug.vectorize(ids).tobytes() == want[ids].tobytes()
    runner.engine.set_clip_pass_bytes(1)                                # one copy per pass
    assert aug.vectorize(ids[:9]).tobytes() == want[ids[:9]].tobytes()
    assert aug.volumes()[2].tolist() == [0] * plan.n_copies
    assert aug.audio(20).tobytes() == expected()[2][20].mix.tobytes()
    with pytest.raises(ValueError):
        aug.vectorize([plan.n_copies])
    aug.close()


def test_a_use_delta_engine_gets_the_delta_columns():
    want = expected_rows()
    clips, noises, copies = expected()
    hpr = P.pr.copy()
    hpr.__dict__['use_delta'] = True
    eng = HipEngine(hpr, synth.make_weights(2 * hpr.n_mfcc, (20,), seed=3))
    aug = NoiseAugmenter(SimpleNamespace(engine=eng), clips, noises)
    aug.load(aug.plan(random.Random(SEED), INFLATION))
    ids = np.array([20, 3, 9, 9, 14, 0, 17], dtype=np.int64)
    got = aug.vectorize(ids)
    assert got.shape == (ids.size, hpr.n_features, 2 * hpr.n_mfcc)
    assert got.tobytes() == np.stack([add_deltas(w) for w in want[ids]]).astype(np.float32).tobytes()
    aug.close()
    eng.close()


def test_append_puts_rows_and_targets_behind_the_resident_set():
    want = expected_rows()
    labels = np.array([0, 1, 0, 1, 1, 0, 1], dtype=np.float32)
    runner = HipRunner(weights=weights())
    aug, plan = planned(runner, labels)
    T, F = P.pr.n_features, P.pr.n_mfcc
    rng = np.random.default_rng(5)
    X = rng.normal(0, 1, (7, T, F)).astype(np.float32)
    y = (rng.random(7) < 0.5).astype(np.float32)
    order = rng.permutation(plan.n_copies)
    ids = np.concatenate([order, order[:4]])
    soft = rng.random(5).astype(np.float32)
    runner.engine.set_clip_pass_bytes(60000 * 4)                        # several passes per call
    for validation in (False, True):
        trainer = Trainer(weights(), ModelParams(recurrent_units=20))
        trainer.set_data(X, y, validation=validation)
        aug.append_to(trainer, validation=validation)                                       # every copy in order, its clip's label
        aug.append_to(trainer, ids, validation=validation)                                  # shuffled and repeated
        aug.append_to(trainer, ids[:5], soft, validation=validation)                        # targets of the caller's
        n = plan.n_copies
        assert trainer.n_samples(validation) == 7 + n + ids.size + 5 and trainer.n_samples(not validation) == 0
        feats, targets = trainer._t.get_data(validation=validation)
        assert feats[:7].tobytes() == X.tobytes() and targets[:7].tobytes() == y.tobytes()
        assert feats[7:7 + n].tobytes() == want.tobytes()
        assert targets[7:7 + n].tobytes() == np.repeat(labels, INFLATION).tobytes()
        assert feats[7 + n:7 + n + ids.size].tobytes() == want[ids].tobytes()
        assert targets[7 + n:7 + n + ids.size].tobytes() == labels[ids // INFLATION].tobytes()
        assert feats[-5:].tobytes() == want[ids[:5]].tobytes() and targets[-5:].tobytes() == soft.tobytes()
        with pytest.raises(ValueError, match=r'targets\[1\]'):
            aug.append_to(trainer, [0, 1], [0.5, 1.5], validation=validation)
        assert trainer.n_samples(validation) == 7 + n + ids.size + 5
        trainer.close()
    with pytest.raises(ValueError, match='no labels'):
        unlabelled, _ = planned(runner)
        unlabelled.append_to(None)
    aug.close()


def test_many_short_copies_run_more_than_one_block_of_chains():
    """280 copies of clips of at most 500 samples: five waves of chains, the last one partly empty, rows of 64 samples that
    cross from one piece into the next, mix blocks that start inside a piece"""
    rng = np.random.default_rng(8)
    lengths = [int(n) for n in rng.integers(1, 501, 70)]
    lengths[:4] = [500, 1, 64, 65]
    clips = [tone(300 + i, n) for i, n in enumerate(lengths)]
    noises = [tone(400 + i, n) for i, n in enumerate((37, 300, 700, 1000, 129))]
    copies = ref.run(clips, ref.Pool(noises), random.Random(21), 4)
    assert len(copies) == 280 and all(ref.out_of_range(c.mix) == 0 and c.noise_volume > 0 for c in copies)
    runner = HipRunner(weights=weights())
    aug = NoiseAugmenter(runner, clips, noises)
    plan = aug.plan(random.Random(21), 4)
    aug.load(plan)
    assert np.count_nonzero(plan.piece_start % 256) > 100 and plan.pieces.size > 400
    va, vn, overflowed = aug.volumes()
    assert va.tobytes() == np.array([copies[4 * c].clip_volume for c in range(70)]).tobytes()
    assert vn.tobytes() == np.array([c.noise_volume for c in copies]).tobytes()
    assert not overflowed.any()
    for o in (0, 1, 2, 3, 4, 63, 64, 127, 128, 255, 256, 279):
        assert aug.pcm(o).tobytes() == ref.saved(copies[o].mix).tobytes(), o
        assert aug.audio(o).tobytes() == copies[o].mix.tobytes(), o
    reloaded = [ref.loaded(ref.saved(c.mix)) for c in copies]
    want = runner.engine.vectorize_clips(reloaded, P.pr.max_samples).astype(np.float32)
    rows = aug.vectorize()
    assert rows.tobytes() == want.tobytes()
    runner.engine.set_clip_pass_bytes(5000 * 4)                         # ten copies or more per pass
    aug.load(plan)
    assert aug.volumes()[1].tobytes() == vn.tobytes() and not aug.volumes()[2].any()
    assert aug.vectorize().tobytes() == rows.tobytes()
    aug.close()


def test_all_zero_noise_under_a_copy_is_refused_and_the_previous_plan_stays():
    clips = [tone(1, 300), tone(2, 700), tone(3, 500)]
    noises = [tone(4, 300), np.zeros(700, np.float32), tone(5, 1000)]
    aug = NoiseAugmenter(HipRunner(weights=weights()), clips, noises)
    aug.noise_id = 2                                                    # from the last recording on: no copy lies in the zeros alone
    good = aug.plan(random.Random(1), 1)
    assert good.cursor == (1, 200, 1)
    aug.load(good)
    before = (aug.volumes(), [aug.audio(o) for o in range(3)], aug.vectorize())
    assert before[0][1][2] > 0 and np.isfinite(before[1][2]).all()     # copy 2 has 200 zeros under it and is fine
    aug.noise_id, aug.noise_pos = 0, 0                                  # from the start: copy 1 takes exactly the zero recording
    bad = aug.plan(random.Random(1), 1)
    assert (int(bad.pieces['noise'][1]), int(bad.pieces['first'][1]), int(bad.pieces['length'][1]), int(bad.copies['n_pieces'][1])) == (1, 0, 700, 1)
    with np.errstate(all='ignore'):
        assert np.isnan(ref.run(clips, ref.Pool(noises), random.Random(1), 1)[1].mix).all()     # what the reference would have saved
    with pytest.raises(ValueError, match='copy 1'):
        aug.load(bad)
    after = (aug.volumes(), [aug.audio(o) for o in range(3)], aug.vectorize())
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before[0], after[0]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before[1], after[1])) and before[2].tobytes() == after[2].tobytes()
    aug.close()


def test_overflowed_counts_the_samples_that_leave_the_int16_range():
    """a loud clip over noise that is quiet but for a few spikes: scaled to the clip's energy the spikes leave the range"""
    rng = np.random.default_rng(6)
    loud = ref.loaded(np.where(np.arange(3000) % 50 < 25, 30000, -30000).astype(np.int16))
    quiet = rng.integers(-40, 41, 5000).astype(np.int16)
    quiet[::250] = 6000
    clips = [tone(7, 1000), loud, tone(8, 800)]
    noises = [ref.loaded(quiet)]
    copies = ref.run(clips, ref.Pool(noises), random.Random(3), 1, 0.3, 0.4)
    counts = [ref.out_of_range(c.mix) for c in copies]
    assert counts[0] == 0 and counts[2] == 0 and 3 <= counts[1] <= 3000 // 250 + 1
    aug = NoiseAugmenter(HipRunner(weights=weights()), clips, noises)
    aug.load(aug.plan(random.Random(3), 1, 0.3, 0.4))
    va, vn, overflowed = aug.volumes()
    assert overflowed.tolist() == counts
    assert vn.tobytes() == np.array([c.noise_volume for c in copies]).tobytes()
    for o in (0, 2):                                                    # the copies beside it are the reference's, byte for byte
        assert aug.pcm(o).tobytes() == ref.saved(copies[o].mix).tobytes()
    assert aug.audio(1).tobytes() == copies[1].mix.tobytes()           # the mix itself is defined; only its cast is not
    aug.close()


def test_write_wavs_writes_the_saved_samples(tmp_path):
    clips, noises = pools((65, 1600), (300, 700))
    aug = NoiseAugmenter(HipRunner(weights=weights()), clips, noises)
    plan = aug.plan(random.Random(2), 2)
    aug.load(plan)
    names = ['wake-word/a.wav', 'wake-word/a.1.wav', 'b.wav', 'b.1.wav']
    aug.write_wavs(str(tmp_path), names)
    for o, name in enumerate(names):
        with wave.open(str(tmp_path / name), 'rb') as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, P.pr.sample_rate)
            assert w.readframes(w.getnframes()) == aug.pcm(o).astype('<i2').tobytes()
    with pytest.raises(ValueError, match='3 names'):
        aug.write_wavs(str(tmp_path), names[:3])
    aug.close()
