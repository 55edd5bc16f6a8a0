"""CPU: the planner of generated training data (mycroft_precise_amd/generated.py) against the restatement of the script's
generators (generated_reference.py): segments, emitted ids, targets and the number of random draws, in both replay modes."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import generated_reference as ref
from conftest import REPO, golden
from mycroft_precise_amd import _build, _lib
from mycroft_precise_amd.generated import Generator, RunLabels

from generated_reference import B, LONG_CLIP, draws, fixture_pools, inputs, tone


class Provenance(ref.Script):
    """the same generators over clips that say where each sample comes from: (pool index + 1) * 2^24 + sample index"""

    def wakeword_sample(self, index, clip, volume):
        return (index + 1) * float(1 << 24) + np.arange(len(clip), dtype=float)


def expected(C, mode, save_draw, script_cls=ref.Script):
    backgrounds, positives, negatives = inputs(C)
    return ref.run(backgrounds, positives, negatives, draws(), C, B, mode=mode, save_draw=save_draw, script_cls=script_cls)


@pytest.mark.parametrize('mode', ['reference', 'tail'])
@pytest.mark.parametrize('C', [512, 1000, 2048])
def test_plan_equals_the_restatement(C, mode):
    backgrounds, positives, negatives = inputs(C)
    per_file, script, n_draws = expected(C, mode, True, Provenance)
    gen = Generator(None, backgrounds, positives, negatives, chunk_size=C)
    plan = gen.plan(ref.CountingRng(draws()), replay=mode)
    assert plan.n_draws == n_draws
    assert plan.chunk_offsets.tolist() == np.concatenate([[0], np.cumsum([len(f) for f in per_file])]).tolist()
    want_ids, want_targets = [], []
    for f, chunks in enumerate(per_file):
        clip, index, target = plan.timeline(f)
        assert clip.size == len(chunks) * C
        seg = plan.files[f]
        assert plan.segments['length'][int(seg['first_segment']):int(seg['first_segment'] + seg['n_segments'])].sum() == len(chunks) * C
        if chunks:
            code = np.concatenate([c[2] for c in chunks]).astype(np.int64)
            assert clip.tolist() == ((code >> 24) - 1).tolist()
            assert index.tolist() == np.where(code > 0, code & ((1 << 24) - 1), 0).tolist()
            assert target.tolist() == np.concatenate([c[3] for c in chunks]).astype(np.int64).tolist()
        for i, _, _, _, got in chunks:
            if got >= 0:
                want_ids.append(int(plan.chunk_offsets[f]) + i)
                want_targets.append(got)
    assert plan.ids.tolist() == want_ids and plan.targets.tolist() == want_targets and plan.targets.dtype == np.float32
    assert len(want_ids) >= 3
    # both clip cycles stand where the script's stand
    n_pos = len(positives)
    assert gen._cycle[1] % n_pos == sum(1 for t in script.taken if t < n_pos) % n_pos
    assert gen._cycle[0] % len(negatives) == sum(1 for t in script.taken if t >= n_pos) % len(negatives)
    # the audio volume and the rms values are the script's Python floats
    assert plan.files['rms'][0] == ref.calc_volume(backgrounds[0])
    assert plan.files['audio_volume'][0] == ref.calc_volume(backgrounds[0]) * (0.4 + 0.5 * 0.37)
    assert np.float32(plan.files['audio_volume'][0]) != plan.files['audio_volume'][0]
    long_segments = plan.segments[plan.segments['clip'] == 0]
    assert long_segments.size and np.all(long_segments['rms'] == ref.calc_volume(positives[0])) and np.all(long_segments['target'] == 1)

    # without the save draw: fewer draws, another stream
    per_file2, _, n_draws2 = expected(C, mode, False)
    gen2 = Generator(None, backgrounds, positives, negatives, chunk_size=C)
    plan2 = gen2.plan(ref.CountingRng(draws()), replay=mode, count_save_draw=False)
    assert plan2.n_draws == n_draws2 < n_draws
    assert plan2.ids.tolist() == [int(plan2.chunk_offsets[f]) + c[0] for f, chunks in enumerate(per_file2) for c in chunks if c[4] >= 0]
    assert plan2.targets.tolist() == [c[4] for chunks in per_file2 for c in chunks if c[4] >= 0]

    # planned file by file (the state -- cycles, run lengths -- carried by the generator), the stream is the same
    gen3 = Generator(None, backgrounds, positives, negatives, chunk_size=C)
    rng = ref.CountingRng(draws())
    parts = [gen3.plan(rng, files=[f], replay=mode) for f in range(len(backgrounds))]
    assert sum(p.n_draws for p in parts) == n_draws
    assert np.concatenate([p.ids + plan.chunk_offsets[f] for f, p in enumerate(parts)]).tolist() == want_ids
    assert np.concatenate([p.targets for p in parts]).tolist() == want_targets
    for f, p in enumerate(parts):
        assert [a.tolist() for a in p.timeline(0)] == [a.tolist() for a in plan.timeline(f)]


def test_the_expected_streams_hold_every_kind_of_chunk():
    """a planner that emits nothing cannot pass: the restatement's own output has a target 1, a target 0 and a skipped chunk"""
    seen = set()
    for C in (512, 1000, 2048):
        for mode in ('reference', 'tail'):
            per_file, _, _ = expected(C, mode, True)
            seen |= {c[4] for chunks in per_file for c in chunks}
    assert seen == {1, 0, -1}


def literal_labels(chunks, buffer_samples):
    vals = np.zeros(buffer_samples, dtype=float)
    out = []
    for pieces in chunks:
        targets = np.concatenate([np.full(n, v, dtype=float) for v, n in pieces])
        vals = np.concatenate((vals[len(targets):], targets))
        out.append(ref.literal_label(vals))
    return out


@pytest.mark.parametrize('buffer_samples,C', [(1, 1), (1, 3), (7, 3), (7, 7), (7, 10), (24000, 2048)])
def test_run_length_labels_equal_the_literal_ones(buffer_samples, C):
    rng = np.random.default_rng(buffer_samples * 31 + C)
    chunks = []
    value = 0
    flip = 0.7 if buffer_samples < 100 else 0.05       # runs around the buffer's length
    for _ in range(400 if buffer_samples < 100 else 250):
        pieces, left = [], C
        while left:
            n = int(min(left, rng.integers(1, 2 * C + 1)))
            pieces.append((value, n))
            left -= n
            if rng.random() < flip:
                value = 1 - value
        chunks.append(pieces)
    labels = RunLabels(buffer_samples)
    got = [labels.push(p) for p in chunks]
    want = literal_labels(chunks, buffer_samples)
    assert got == want
    assert len(set(want)) >= 2 and (buffer_samples < 100 or set(want) == {1, 0, -1})


def test_a_run_of_exactly_eight_tenths_and_of_exactly_half_the_buffer():
    C = 2400
    chunks = [[(1, C)]] * 8 + [[(0, C)]] * 6           # 19200 ones, then zeros push them out 2400 at a time
    labels = RunLabels(B)
    got = [labels.push(p) for p in chunks]
    assert got == literal_labels(chunks, B)
    assert got[8] == -1         # 19200 / 24000 is not > 0.8
    assert got[9] == -1 and got[10] == -1 and got[11] == -1
    assert got[12] == -1        # 12000 / 24000 is not < 0.5
    assert got[13] == 0
    one_more = [[(0, C - 1), (1, 1)]] + chunks          # 19201 ones
    labels = RunLabels(B)
    got = [labels.push(p) for p in one_more]
    assert got == literal_labels(one_more, B) and got[9] == 1


def test_labels_depend_on_the_previous_files_tail():
    positives, negatives = [tone(1, 9)], [tone(2, 3)]
    backgrounds = [tone(3, 14), tone(4, 14)]
    kw = dict(chunk_size=4, buffer_samples=11, sample_rate=4)
    differing = 0
    for seed in range(40):
        r = random.Random(seed)
        d = [r.random() for _ in range(200)]
        per_file, _, n_draws = ref.run(backgrounds, positives, negatives, d, 4, 11, sample_rate=4)
        gen = Generator(None, backgrounds, positives, negatives, **kw)
        rng = ref.CountingRng(d)
        first, second = gen.plan(rng, files=[0]), gen.plan(rng, files=[1])
        assert first.n_draws + second.n_draws == n_draws
        for plan, chunks in ((first, per_file[0]), (second, per_file[1])):
            assert plan.ids.tolist() == [c[0] for c in chunks if c[4] >= 0]
            assert plan.targets.tolist() == [c[4] for c in chunks if c[4] >= 0]
        # the same second file, drawn the same way, behind nothing: other labels whenever the first file ended in a wake word
        alone, _, _ = ref.run(backgrounds[1:], positives, negatives, d[first.n_draws:], 4, 11, sample_rate=4)
        differing += [c[4] for c in alone[0]] != [c[4] for c in per_file[1]]
    assert differing >= 1


def test_reference_replay_differs_from_tail():
    C = 512
    backgrounds, positives, negatives = inputs(C)
    plans = {mode: Generator(None, backgrounds, positives, negatives, chunk_size=C).plan(ref.CountingRng(draws()), files=[0], replay=mode)
             for mode in ('reference', 'tail')}
    assert LONG_CLIP > C
    a, b = plans['reference'].timeline(0), plans['tail'].timeline(0)
    assert a[0].size == b[0].size and (a[0].tolist() != b[0].tolist() or a[1].tolist() != b[1].tolist())
    # 'reference' plays the long clip from its start a second time; 'tail' goes on to its last samples and into the silence
    k = ((LONG_CLIP - 1) // C) * C
    assert a[1][k] == 0 and a[0][k] == 0 and b[1][k] == k and b[0][k + (LONG_CLIP - k)] == -1


def test_refusals():
    good = tone(1, 100)
    with pytest.raises(ValueError, match=r'negatives\[1\]'):
        Generator(None, [good], [good], [good, np.zeros(50, np.float32)])
    with pytest.raises(ValueError, match='hey'):
        Generator(None, [good], {'hey': np.zeros(0, np.float32)}, [good])
    gen = Generator(None, [good, np.zeros(5000, np.float32), np.zeros(10, np.float32)], [good], [good], chunk_size=512)
    with pytest.raises(ValueError, match='replay'):
        gen.plan(random.Random(1), replay='both')
    with pytest.raises(ValueError, match=r'backgrounds\[1\]'):
        gen.plan(random.Random(1), files=[1])
    plan = gen.plan(random.Random(1), files=[2])         # no chunk: skipped after its volume draw, silent or not
    assert plan.n_draws == 1 and plan.n_chunks == 0 and plan.ids.size == 0


def test_the_generator_symbols_are_declared_and_exported():
    text = open(os.path.join(REPO, 'include', 'precise_engine.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = sorted(set(re.findall(r'\b(pe_generator_[a-z_0-9]+)\s*\(', text)))
    assert names == ['pe_generator_append', 'pe_generator_audio', 'pe_generator_create', 'pe_generator_destroy', 'pe_generator_set_plan',
                     'pe_generator_vectorize']
    raw = ctypes.CDLL(_build.build())
    for n in names:
        assert hasattr(raw, n) and n in _lib.EXPORTS
    assert _lib.GEN_FILE.itemsize == 40 and _lib.GEN_SEGMENT.itemsize == 40


# ---- the script itself: tests/golden/train_generated.npz (tools/make_script_fixtures.py) --------------------------------------
def restated_stream(g, C, mode='reference', save_draw=True):
    """the restatement over the fixture's pools and draws, in the fixture's own terms"""
    from oracle import listener as ol
    backgrounds, positives, negatives, draws = fixture_pools(g, C)
    rng = ref.CountingRng(draws)
    script = ref.Script(positives, negatives, rng, C, int(g['buffer_samples']), mode=mode, save_draw=save_draw)
    lis = ol.OracleListener(None)
    keep = set(g['audio_ids_%d' % C].tolist())
    out = {name: [] for name in ('label', 'ones', 'last', 'max_run', 'vals_len', 'file_draws', 'file_taken', 'audio', 'windows')}
    chunk_offsets = [0]
    for audio in backgrounds:
        draws_before, taken_before, n = rng.n, len(script.taken), 0
        lis.clear()
        for i, chunk, _, targets, label in script.vectors_from(audio):
            window = lis.update_vectors(chunk)
            out['label'].append(label)
            out['ones'].append(int(np.count_nonzero(targets == 1)))
            out['last'].append(int(script.vals_buffer[-1]))
            out['max_run'].append(int(ref.max_run_length(script.vals_buffer, 1)))
            out['vals_len'].append(len(script.vals_buffer))
            if chunk_offsets[-1] + i in keep:
                assert chunk.dtype == np.float64
                out['audio'].append(chunk)
            if label >= 0:
                out['windows'].append(window)
            n += 1
        chunk_offsets.append(chunk_offsets[-1] + n)
        out['file_draws'].append(rng.n - draws_before)
        out['file_taken'].append(len(script.taken) - taken_before)
    out['chunk_offsets'], out['taken'] = chunk_offsets, script.taken
    return out


def stream_differences(g, C, got):
    """the names of the fixture's arrays the restated stream does not reproduce exactly"""
    k = '_%d' % C
    bad = [name for name in ('label', 'ones', 'last', 'max_run', 'vals_len', 'file_draws', 'file_taken', 'chunk_offsets', 'taken')
           if g[name + k].tolist() != list(got[name])]
    audio = np.concatenate(got['audio']) if got['audio'] else np.zeros(0)
    if audio.tobytes() != g['audio' + k].tobytes():
        bad.append('audio')
    windows = np.array(got['windows']).reshape(-1, 29, 13)
    if not np.array_equal(windows, g['windows' + k]):          # (equality: what test_oracle.py asks of the Listener's ring)
        bad.append('windows')
    return bad


@pytest.mark.parametrize('C', [512, 2048])
def test_restatement_and_planner_equal_the_scripts_own_stream(C):
    """TrainGeneratedScript.vectors_from_fn itself, over five background files on one script object: labels, draws per file,
    clips pulled, run summaries, merged audio bits and the emitted windows."""
    g = golden('train_generated.npz')
    k = '_%d' % C
    labels = g['label' + k]
    assert set(labels.tolist()) == {1, 0, -1} and g['audio_ids' + k].size >= 10 and g['windows' + k].shape[0] == np.count_nonzero(labels >= 0)
    lengths = np.diff(g['background_offsets' + k]).tolist()
    clip_lengths = np.diff(g['clip_offsets' + k]).tolist()
    assert C + 1 in lengths and 2 * C + 1 in lengths and C in clip_lengths and C - 1 in clip_lengths and max(clip_lengths) > 0.8 * B
    assert stream_differences(g, C, restated_stream(g, C)) == []
    # the wrong readings: each must fail against the fixture
    tail = stream_differences(g, C, restated_stream(g, C, mode='tail'))
    assert 'audio' in tail and 'label' in tail, tail
    no_save = stream_differences(g, C, restated_stream(g, C, save_draw=False))
    assert 'file_draws' in no_save, no_save
    # the planner over the same pools and draws
    backgrounds, positives, negatives, draws = fixture_pools(g, C)
    plan = Generator(None, backgrounds, positives, negatives, chunk_size=C).plan(ref.CountingRng(draws))
    assert plan.n_draws == int(g['file_draws' + k].sum()) and plan.chunk_offsets.tolist() == g['chunk_offsets' + k].tolist()
    assert plan.ids.tolist() == np.flatnonzero(labels >= 0).tolist() and plan.targets.tolist() == labels[labels >= 0].tolist()
    for mode, save in (('tail', True), ('reference', False)):
        other = Generator(None, backgrounds, positives, negatives, chunk_size=C).plan(ref.CountingRng(draws), replay=mode, count_save_draw=save)
        assert other.n_draws != plan.n_draws or other.ids.tolist() != plan.ids.tolist() or other.targets.tolist() != plan.targets.tolist()
