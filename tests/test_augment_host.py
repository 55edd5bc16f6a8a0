"""CPU: the planner of noise augmentation (mycroft_precise_amd/augment.py) against the restatement of the script's noise pool
(augment_reference.py), the restatement against what the reference's own code computed (tests/golden/add_noise.npz), and every
refusal of pe_augmenter_set_plan through a session without a device."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import augment_reference as ref
from conftest import REPO, golden
from mycroft_precise_amd import _build, _lib
from mycroft_precise_amd.augment import NoiseAugmenter

INVALID = 1


def tone(seed, n, amplitude=8000):
    """what load_audio returns for an int16 recording: float32(int16) / 32767"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.6 * np.sin(2 * np.pi * t * rng.uniform(0.01, 0.2)) + 0.4 * rng.uniform(-1.0, 1.0, n)
    return ref.loaded(np.round(amplitude * x).astype(np.int16))


def pools(clip_lengths, noise_lengths):
    return [tone(100 + i, n) for i, n in enumerate(clip_lengths)], [tone(200 + i, n) for i, n in enumerate(noise_lengths)]


def check_plan(plan, copies):
    """the planner's tables against the restatement's copies"""
    assert plan.n_copies == len(copies)
    assert plan.copies['clip'].tolist() == [c.clip for c in copies]
    assert plan.copies['ratio'].tobytes() == np.array([c.ratio for c in copies], dtype=np.float64).tobytes()
    assert plan.copies['first_piece'].tolist() == np.concatenate([[0], np.cumsum([len(c.steps) for c in copies])])[:-1].tolist()
    assert plan.copies['n_pieces'].tolist() == [len(c.steps) for c in copies]
    steps = [s for c in copies for s in c.steps]
    assert list(zip(plan.pieces['noise'].tolist(), plan.pieces['first'].tolist(), plan.pieces['length'].tolist())) == steps
    assert plan.piece_copy.tolist() == [o for o, c in enumerate(copies) for _ in c.steps]
    assert plan.piece_start.tolist() == [int(x) for c in copies for x in np.concatenate([[0], np.cumsum([s[2] for s in c.steps])])[:-1]]
    assert plan.cursor == copies[-1].cursor


# clip lengths, noise lengths, inflation factor, what the case is there for
CASES = [
    ((1, 65, 1599, 1600, 2401), (1, 300, 700, 1000), 3, 'several'),     # pieces over one and several recordings, many wraps
    ((100, 50, 150, 30), (100, 50), 1, 'exact'),                         # slices that end exactly at a recording's end
    ((40, 10, 7), (1000,), 2, 'inside'),                                 # every copy inside one recording: no wrap at all
    ((5000,), (300, 700, 1000), 2, 'wraps'),                             # one copy walks the whole pool more than twice
]


@pytest.mark.parametrize('clip_lengths,noise_lengths,inflation,what', CASES, ids=[c[3] for c in CASES])
def test_plan_equals_the_restatement(clip_lengths, noise_lengths, inflation, what):
    clips, noises = pools(clip_lengths, noise_lengths)
    pool = ref.Pool(noises)
    draws = ref.CountingRng(random.Random(11))
    copies = ref.run(clips, pool, draws, inflation, 0.1, 0.35)
    aug = NoiseAugmenter(None, clips, noises)
    plan = aug.plan(random.Random(11), inflation, 0.1, 0.35)
    check_plan(plan, copies)
    assert plan.n_draws == draws.n == len(clips) * inflation and plan.inflation_factor == inflation
    assert plan.clip.tolist() == [o // inflation for o in range(plan.n_copies)]
    per_copy = plan.copies['n_pieces']
    if what == 'several':
        assert per_copy.min() == 1 and per_copy.max() >= 4 and plan.cursor[2] >= 3
        assert np.any(plan.pieces['first'] > 0)                         # a copy that starts inside a recording
    if what == 'exact':
        # the first copy takes recording 0 whole, the second recording 1 whole, the third both: the cursor is back at the start
        assert list(zip(plan.pieces['noise'].tolist(), plan.pieces['first'].tolist(), plan.pieces['length'].tolist()))[:4] == \
            [(0, 0, 100), (1, 0, 50), (0, 0, 100), (1, 0, 50)]
        assert copies[0].cursor == (1, 0, 0) and copies[1].cursor == (0, 0, 1) and copies[2].cursor == (0, 0, 2)
        assert plan.cursor == (0, 30, 2)
    if what == 'inside':
        assert per_copy.tolist() == [1] * 6 and plan.cursor == (0, 114, 0)
    if what == 'wraps':
        # 5000 = 2 * 2000 + 300 + 700: eight pieces; then from recording 2 on 1000 + 2 * 2000: seven, ending at the pool's end
        assert per_copy.tolist() == [8, 7] and copies[0].cursor == (2, 0, 2) and plan.cursor == (0, 0, 5)


def test_the_cursor_lives_on_across_plan_calls():
    clips, noises = pools((1, 65, 1599, 1600, 2401), (1, 300, 700, 1000))
    pool = ref.Pool(noises)
    rng = random.Random(5)
    first = ref.run(clips, pool, rng, 2)
    second = ref.run(clips[::-1], pool, rng, 1, 0.2, 0.9)
    aug = NoiseAugmenter(None, clips, noises)
    other = NoiseAugmenter(None, clips[::-1], noises)
    rng = ref.CountingRng(random.Random(5))
    plan = aug.plan(rng, 2)
    check_plan(plan, first)
    assert first[-1].cursor != (0, 0, 0) and rng.n == 10
    other.noise_id, other.noise_pos, other.repeat_count = plan.cursor          # the script's NoiseData goes on where it stood
    again = other.plan(rng, 1, 0.2, 0.9)
    check_plan(again, second)
    assert rng.n == 15 and again.cursor == second[-1].cursor
    # the same augmenter planned twice: the second plan starts where the first ended, not at the pool's start
    twice = aug.plan(random.Random(1), 1)
    fresh = NoiseAugmenter(None, clips, noises).plan(random.Random(1), 1)
    assert (int(twice.pieces['noise'][0]), int(twice.pieces['first'][0])) == plan.cursor[:2] != (0, 0)
    assert (int(fresh.pieces['noise'][0]), int(fresh.pieces['first'][0])) == (0, 0)
    assert twice.cursor[2] > plan.cursor[2]
    assert aug.plan(random.Random(1), 0).n_copies == 0


def fixture_pools(g):
    split = lambda pcm, off: [ref.loaded(pcm[a:b]) for a, b in zip(off[:-1], off[1:])]
    return split(g['clip_pcm'], g['clip_offsets']), split(g['noise_pcm'], g['noise_offsets'])


def test_the_restatement_equals_the_reference(capsys):
    """the fixture holds what the reference's own NoiseData, load_audio and save_audio computed: mixes, saved samples, cursors"""
    g = golden('add_noise.npz')
    print('provenance:', '; '.join(str(p) for p in g['provenance']))
    assert any('add_noise.py' in str(p) and 'unmodified' in str(p) for p in g['provenance'])
    clips, noises = fixture_pools(g)
    assert all(c.dtype == np.float32 for c in clips + noises)
    inflation = int(g['inflation_factor'])
    copies = ref.run(clips, ref.Pool(noises), random.Random(int(g['seed'])), inflation)
    assert [c.clip for c in copies] == g['clip'].tolist() and len(copies) == 10
    assert np.array([c.ratio for c in copies]).tobytes() == g['ratio'].tobytes()
    assert [list(c.cursor) for c in copies] == g['cursor'].tolist()
    mixed = np.concatenate([c.mix for c in copies])
    assert mixed.dtype == np.float64 and mixed.tobytes() == g['mixed'].tobytes()
    assert np.concatenate([ref.saved(c.mix) for c in copies]).tobytes() == g['saved'].tobytes()
    assert sum(ref.out_of_range(c.mix) for c in copies) == 0 and np.abs(mixed).max() < 0.25
    assert g['cursor'][-1][2] >= 1                                      # the pool was walked through more than once
    # ... and the planner stands where the reference's cursor stood
    plan = NoiseAugmenter(None, clips, noises).plan(random.Random(int(g['seed'])), inflation)
    check_plan(plan, copies)
    assert list(plan.cursor) == g['cursor'][-1].tolist()


def test_the_sums_are_chains_in_the_arrays_own_type():
    """what the device is held to: a float32 chain over the clip, a float64 chain over the noise -- neither is numpy's pairwise sum"""
    clips, noises = pools((2401,), (300, 700, 1000))
    copy = ref.run(clips, ref.Pool(noises), random.Random(2), 1)[0]
    s = np.float32(0.0)
    for x in clips[0]:
        s = np.float32(s + np.float32(x * x))
    assert copy.clip_volume == float(np.sqrt(np.float64(s)))
    noise = np.concatenate([noises[r][a:a + n] for r, a, n in copy.steps]).astype(np.float64)
    d = 0.0
    for x in noise:
        d += float(x) * float(x)
    assert copy.noise_volume == float(np.sqrt(d))
    assert copy.clip_volume != float(np.sqrt(np.sum(clips[0].astype(np.float64) ** 2)))


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_the_planner_refuses_empty_recordings_by_name():
    good = tone(1, 100)
    with pytest.raises(ValueError, match=r'clips\[1\] is empty'):
        NoiseAugmenter(None, [good, np.zeros(0, np.float32)], [good])
    with pytest.raises(ValueError, match=r'noise recording hiss is empty'):
        NoiseAugmenter(None, [good], {'hum': good, 'hiss': np.zeros(0, np.float32)})
    with pytest.raises(ValueError, match='no noise'):
        NoiseAugmenter(None, [good], [])
    with pytest.raises(ValueError, match='float32'):
        NoiseAugmenter(None, [good.astype(np.float64)], [good])
    with pytest.raises(ValueError, match='3 labels for 1 clips'):
        NoiseAugmenter(None, [good], [good], labels=[0, 1, 1])
    aug = NoiseAugmenter(None, [good], [good])
    with pytest.raises(ValueError, match='no plan'):
        aug.audio(0)


def test_set_plan_refuses_every_broken_plan_by_name():
    """a session created without an engine runs pe_augmenter_set_plan's host checks and nothing else"""
    clips, noises = pools((65, 1599, 700), (300, 700, 1000))
    plan = NoiseAugmenter(None, clips, noises).plan(random.Random(3), 2)
    session = _lib.HipAugmenter(None, clips, noises)
    lib, h = session._lib, session._h
    err = lambda: lib.pe_last_global_error().decode()
    session.set_plan(plan.copies, plan.pieces)                          # the planner's own plan passes
    assert session.n_copies == 6

    def refused(copies, pieces, word, n_pieces=None):
        rc = lib.pe_augmenter_set_plan(h, copies.ctypes.data, copies.size, pieces.ctypes.data, pieces.size if n_pieces is None else n_pieces)
        assert rc == INVALID and word in err(), err()

    def broken(table, field, row, value):
        bad = table.copy()
        bad[field][row] = value
        return bad

    copies, pieces = plan.copies, plan.pieces
    two = int(copies['first_piece'][2])                                 # the first piece of copy 2
    assert copies['n_pieces'][2] >= 2
    refused(broken(copies, 'clip', 1, 3), pieces, 'copy 1 names clip 3 of 3')
    refused(broken(copies, 'clip', 1, -1), pieces, 'copy 1 names clip -1')
    refused(copies, broken(pieces, 'noise', two, 3), 'piece %d names noise recording 3 of 3' % two)
    refused(copies, broken(pieces, 'noise', two, -1), 'piece %d names noise recording -1' % two)
    first, length = int(pieces['first'][two]), int(pieces['length'][two])
    rec_len = len(noises[int(pieces['noise'][two])])
    refused(copies, broken(pieces, 'first', two, rec_len - length + 1), 'piece %d takes samples %d + %d of noise recording' % (two, rec_len - length + 1, length))
    refused(copies, broken(pieces, 'first', two, -1), 'piece %d takes samples -1' % two)
    refused(copies, broken(pieces, 'length', two, 0), 'piece %d has length 0' % two)
    refused(copies, broken(pieces, 'length', two, -5), 'piece %d has length -5' % two)
    end = two + int(copies['n_pieces'][2]) - 1                          # the last piece of copy 2 ends inside its recording
    assert int(pieces['first'][end] + pieces['length'][end]) < len(noises[int(pieces['noise'][end])])
    refused(copies, broken(pieces, 'length', end, int(pieces['length'][end]) + 1), 'the pieces of copy 2 overrun the 1599 samples of its clip 1 at piece %d' % end)
    refused(copies, broken(pieces, 'length', two, length - 1), 'the pieces of copy 2 hold %d samples, its clip 1 has 1599' % (1599 - 1))
    last = pieces.size - 1
    refused(copies, broken(pieces, 'length', last, int(pieces['length'][last]) - 1), 'the pieces of copy 5 hold 699 samples, its clip 2 has 700')
    refused(broken(copies, 'first_piece', 3, int(copies['first_piece'][3]) + 1), pieces, 'copy 3 takes pieces')
    refused(broken(copies, 'n_pieces', 5, int(copies['n_pieces'][5]) + 1), pieces, 'copy 5 takes pieces')
    refused(broken(copies, 'n_pieces', 4, -1), pieces, 'copy 4 takes pieces')
    refused(broken(copies, 'ratio', 4, np.nan), pieces, 'copy 4 has ratio NaN')
    more = np.concatenate([pieces, pieces[-1:]])
    refused(copies, more, 'the copies take %d of %d pieces' % (pieces.size, pieces.size + 1))
    refused(copies, pieces, 'more than 2^31 - 1', n_pieces=1 << 31)
    assert lib.pe_augmenter_set_plan(h, None, 2, pieces.ctypes.data, pieces.size) == INVALID and 'null argument' in err()
    assert lib.pe_augmenter_set_plan(h, copies.ctypes.data, -1, pieces.ctypes.data, pieces.size) == INVALID
    # through the wrapper the same refusals are ValueErrors, and the plan that was set stays
    with pytest.raises(ValueError, match='copy 1 names clip 3'):
        session.set_plan(broken(copies, 'clip', 1, 3), pieces)
    assert session.n_copies == 6
    # everything that needs the device says so
    for call in (lambda: session.volumes(), lambda: session.audio(0), lambda: session.pcm(0)):
        with pytest.raises(ValueError, match='without an engine'):
            call()
    ids = np.zeros(1, np.int32)
    out = np.zeros(4096, np.float32)
    assert lib.pe_augmenter_vectorize(h, ids.ctypes.data, 1, 0, out.ctypes.data) == INVALID and 'without an engine' in err()
    assert lib.pe_augmenter_append(h, None, 0, ids.ctypes.data, out.ctypes.data, 1, 0) == INVALID and 'without an engine' in err()
    session.close()
    with pytest.raises(ValueError, match='closed'):
        session.set_plan(copies, pieces)


def test_create_refuses_empty_recordings_by_name():
    lib = _lib.load()
    h = ctypes.c_void_p()
    audio = np.zeros(10, np.float32)
    off = lambda *v: np.array(v, dtype=np.int64)
    create = lambda co, no: lib.pe_augmenter_create(None, audio.ctypes.data, co.ctypes.data, co.size - 1, audio.ctypes.data, no.ctypes.data,
                                                    no.size - 1, ctypes.byref(h))
    err = lambda: lib.pe_last_global_error().decode()
    assert create(off(0, 4, 4, 10), off(0, 10)) == INVALID and err() == 'pe_augmenter_create: clip 1 is empty' and not h.value
    assert create(off(0, 4, 10), off(0, 0, 10)) == INVALID and 'noise recording 0 is empty' in err()
    assert create(off(0, 4, 10), off(0)) == INVALID and err() == 'pe_augmenter_create: 0 noise recordings (at least one is needed)'
    assert create(off(0), off(0, 10)) == INVALID and '0 clips' in err()
    assert create(off(1, 4), off(0, 10)) == INVALID and err() == 'pe_augmenter_create: clip offsets[0] must be 0, got 1'
    assert create(off(0, 4, 2), off(0, 10)) == INVALID and err() == 'pe_augmenter_create: offsets decrease at clip 1 (2 after 4)'
    assert lib.pe_augmenter_create(None, audio.ctypes.data, off(0, 4).ctypes.data, 1, audio.ctypes.data, off(0, 10).ctypes.data, 1, None) == INVALID
    assert create(off(0, 4, 10), off(0, 10)) == 0 and h.value
    assert lib.pe_augmenter_destroy(h) == 0
    # a null session is refused before anything is read, whatever else is null
    assert lib.pe_miner_vectorize(None, None, 0, None) == INVALID
    assert lib.pe_generator_append(None, None, 0, None, None, 0) == INVALID
    assert lib.pe_augmenter_append(None, None, 0, None, None, 0, 0) == INVALID


def test_the_augmenter_symbols_are_declared_and_exported():
    text = open(os.path.join(REPO, 'include', 'precise_engine.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = sorted(set(re.findall(r'\b(pe_augmenter_[a-z_0-9]+)\s*\(', text)))
    assert names == ['pe_augmenter_append', 'pe_augmenter_audio', 'pe_augmenter_create', 'pe_augmenter_destroy', 'pe_augmenter_set_plan',
                     'pe_augmenter_vectorize', 'pe_augmenter_volumes']
    raw = ctypes.CDLL(_build.build())
    for n in names:
        assert hasattr(raw, n) and n in _lib.EXPORTS
    assert _lib.AUG_COPY.itemsize == 32 and _lib.AUG_PIECE.itemsize == 24
    assert raw.pe_abi_version() == 8
