"""
The chain launch's prologue (csrc/gru_chain_device.h: gru_tile_chains): the new rows are projected once per workgroup -- a tile
of the projections per wave -- and handed round through an LDS mailbox behind one workgroup barrier.  That changes no bit: as in
test_chain_carry, the reference of every comparison is the same engine class with set_chain_carry(0), fed the same chunks, and
the comparison is np.array_equal on every update's output and on the feature windows afterwards.  No tolerance appears
anywhere.
"""
import numpy as np
import pytest

from mycroft_precise_amd import synth
from mycroft_precise_amd import params as P

pytestmark = pytest.mark.gpu


def _engine(weights, n, mode, **kw):
    from mycroft_precise_amd._lib import HipEngine
    e = HipEngine(P.pr, weights, n_streams=n, **kw)
    e.set_chain_carry(mode)
    return e


def _weights(seed=42):
    return synth.make_weights(n_in=P.pr.n_mfcc, units=(20,), seed=seed)


def _audio(n, total, first=0):
    """int16 [n][total]: tones in noise, and -- the last three streams -- silence, a full-scale square wave, a quiet stream"""
    kinds = ['tone_noise'] * (n - 3) + ['zeros', 'square', 'quiet']
    return np.stack([synth.stream_pcm(first + s, total, k) for s, k in enumerate(kinds)])


def _emitted(pos):
    """rows visible to the network after `pos` samples of a stream"""
    pos = np.asarray(pos, dtype=np.int64)
    return np.where(pos >= P.pr.window_samples, 1 + (pos - P.pr.window_samples) // P.pr.hop_samples, 0)


# 1024: k = 1 and k = 2 mixed; 400: k = 0 and k = 1 (a tile in which nothing became visible skips the projection, the barrier and
# the chains altogether); the alternation: k = 0, 1 and 2 in one run.  More than two wraps of the 32-slot ring each.
SEQS = {'1024': [1024] * 60, '400': [400] * 150, '400_1024': [400, 1024] * 45}


def _run_sequence(n, chunks, **kw):
    w = _weights()
    audio = _audio(n, sum(chunks))
    ref, eng = _engine(w, n, 0, **kw), _engine(w, n, 2, **kw)
    pos, ks = 0, set()
    for u, c in enumerate(chunks):
        pcm = audio[:, pos:pos + c]
        if _emitted(pos) > 0:                                      # (past the start-up: the first window needs 1600 samples)
            ks.add(int(_emitted(pos + c) - _emitted(pos)))
        pos += c
        want, got = ref.update(pcm), eng.update(pcm)
        assert np.array_equal(got, want), (u, c, np.flatnonzero(got != want)[:8])
        assert eng.chain_carry() == (2, True), u
    assert _emitted(pos) > 2 * 32
    assert np.array_equal(ref.get_vectors(), eng.get_vectors())
    ref.close(); eng.close()
    return ks


@pytest.mark.parametrize('seq', list(SEQS))
@pytest.mark.parametrize('n', [16, 17, 70])
def test_stream_counts_and_chunk_sequences(n, seq):
    """one full tile; a second tile with one valid lane; four tiles and six lanes of a fifth"""
    ks = _run_sequence(n, SEQS[seq])
    assert ks == {'1024': {1, 2}, '400': {0, 1}, '400_1024': {0, 1, 2}}[seq]


def test_float32_front_end():
    """the _nopk twin of the kernel, whose workgroups have half the LDS (the mailbox must fit in it)"""
    assert _run_sequence(17, SEQS['400_1024'], mfcc_precision='f32') == {0, 1, 2}


def test_lanes_of_one_tile_with_different_k():
    """64 streams at four private phases; half of every tile of 16 gets an extra 400 samples every third call.  Calls alternate
    between a permutation of all streams (four waves per tile) and a random half of them (a sparse subset: eight waves per tile,
    two workgroups); the tiles of a call are runs of 16 of ITS ids, so their lanes differ in emitted count and in k.  Counted here
    from the sample positions: both shapes must have met tiles with mixed k."""
    n, n_calls = 64, 90
    w = _weights()
    rng = np.random.default_rng(20261020)
    audio = _audio(n, n_calls * 1024 + 4000)
    ref, eng = _engine(w, n, 0), _engine(w, n, 2)
    pos = np.zeros(n, dtype=np.int64)

    def call(ids, chunk):
        ids = np.asarray(ids)
        pcm = np.stack([audio[s, pos[s]:pos[s] + chunk] for s in ids])
        want, got = ref.update_subset(ids, pcm), eng.update_subset(ids, pcm)
        assert np.array_equal(got, want), (chunk, np.flatnonzero(got != want)[:8])
        k = _emitted(pos[ids] + chunk) - _emitted(pos[ids])
        pos[ids] += chunk
        pad = np.concatenate([k, np.full(-len(k) % 16, k[0])]).reshape(-1, 16)
        return sum(len(set(t)) > 1 for t in pad)

    for r in range(4):                                             # private phases: 0, 200, 400, 600 samples into the hop
        if r:
            call(np.arange(r, n, 4), 200 * r)
    assert eng.chain_carry() == (2, True)
    slow = np.flatnonzero(np.arange(n) % 16 >= 8)
    mixed = {4: 0, 8: 0}
    for i in range(n_calls):
        chunk = (400, 1024, 800)[i % 3]
        if i % 2 == 0:
            nw, ids = 4, rng.permutation(n)
        else:
            nw, ids = 8, rng.permutation(n)[:n // 2]
        mixed[nw] += call(ids, chunk)
        if i % 3 == 2:
            call(slow, 400)
        assert eng.chain_carry() == (2, True), i
    assert mixed[4] >= 20 and mixed[8] >= 20, mixed
    assert np.array_equal(ref.get_vectors(), eng.get_vectors())
    ref.close(); eng.close()


def test_stale_lds_of_another_engine():
    """two engines with different weights and different audio take turns on one device: the chain workgroups of one inherit the
    LDS the other's left behind in the mailbox, and read none of it: each engine's outputs are those of its own solo
    run, which are those of the plain launch"""
    n = 17
    chunks = SEQS['400_1024'][:50]
    nets = [_weights(seed=42), _weights(seed=7)]
    audios = [_audio(n, sum(chunks)), _audio(n, sum(chunks), first=100)[:, ::-1].copy()]
    solo = []
    for w, audio in zip(nets, audios):
        ref, eng = _engine(w, n, 0), _engine(w, n, 2)
        outs, pos = [], 0
        for c in chunks:
            outs.append(eng.update(audio[:, pos:pos + c]).copy())
            assert np.array_equal(outs[-1], ref.update(audio[:, pos:pos + c]))
            pos += c
        solo.append((outs, eng.get_vectors()))
        ref.close(); eng.close()
    assert not np.array_equal(solo[0][0][-1], solo[1][0][-1])
    engs = [_engine(w, n, 2) for w in nets]
    pos = 0
    for u, c in enumerate(chunks):
        for e in (0, 1):
            assert np.array_equal(engs[e].update(audios[e][:, pos:pos + c]), solo[e][0][u]), (u, e)
            assert engs[e].chain_carry() == (2, True)
        pos += c
    for e in (0, 1):
        assert np.array_equal(engs[e].get_vectors(), solo[e][1])
        engs[e].close()
