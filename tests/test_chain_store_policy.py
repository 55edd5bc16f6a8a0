"""
How a chain launch stores what the NEXT launch reads (csrc/gru_chain_device.h: chain_store; the rebuild kernel shares it).  A
chain's cell is loaded and stored by one wave of one launch, and its next reader is a later launch behind a kernel boundary, so
the policy of the store (plain, written through the L2, non-temporal) may change no bit.  The cases here are the ones in which that
next reader is NOT the compute unit that wrote the cell: consecutive calls that alternate between one workgroup per tile (a full
update, gru_tile_chains<4>) and two (a subset of at most half of the engine's streams, <8>: other workgroup indices), a rebuild
kernel in between, the instantiation that leaves chains out, and an output that lies in pinned host memory.

The reference of every comparison is a second engine with set_chain_carry(0), fed the same audio, compared with np.array_equal
after every call.  No tolerance appears, nothing is timed, no assembly is read.
"""
import numpy as np
import pytest

from mycroft_precise_amd import synth
from mycroft_precise_amd import params as P

pytestmark = pytest.mark.gpu

N_SKIP = 128                                # eligible calls in a row with one chunk > hop before chains are left out (precise_engine.h)
CHUNKS = [160, 480, 800, 1024, 1088]        # 0, 0 or 1, 1, 1 or 2, 1 or 2 rows per update (hop 800)
FRONTS = ['f64', 'f32']
TILE = 16


def _weights(seed=42):
    return synth.make_weights(n_in=P.pr.n_mfcc, units=(20,), seed=seed)


def _audio(n, total):
    kinds = ['tone_noise'] * (n - 3) + ['zeros', 'square', 'quiet']
    return np.stack([synth.stream_pcm(s, total, k) for s, k in enumerate(kinds)])


def _sparse_size(n):
    """the most streams a subset call may name and still get two workgroups per tile (kernels.hip launch_fused_chains_t: twice
    the call's streams, rounded up to tiles, fit the engine's padded stream count), and at most half of the engine's streams"""
    n_padded = -(-n // TILE) * TILE
    return min(n // 2, (n_padded // (2 * TILE)) * TILE)


class Pair:
    """the reference engine (chains off) and the engine under test (chains eager), fed alike"""

    def __init__(self, n, front, seed):
        from mycroft_precise_amd._lib import HipEngine
        self.n = n
        w = _weights()
        self.ref = HipEngine(P.pr, w, n_streams=n, mfcc_precision=front)
        self.eng = HipEngine(P.pr, w, n_streams=n, mfcc_precision=front)
        self.ref.set_chain_carry(0)
        self.eng.set_chain_carry(2)
        self.pos = np.zeros(n, dtype=np.int64)
        self.rng = np.random.default_rng(seed)
        self.n_sub = _sparse_size(n)
        assert 0 < 2 * self.n_sub <= n
        self.rows = set()                   # rows per stream and call that the calls made visible

    def take(self, audio, ids, chunk):
        pcm = np.stack([audio[s, self.pos[s]:self.pos[s] + chunk] for s in ids])
        before = np.maximum(0, 1 + (self.pos[ids] - P.pr.window_samples) // P.pr.hop_samples)
        self.pos[ids] += chunk
        after = np.maximum(0, 1 + (self.pos[ids] - P.pr.window_samples) // P.pr.hop_samples)
        self.rows |= set(int(k) for k in after - before)
        return np.ascontiguousarray(pcm)

    def same(self, got, want, tag):
        assert not np.isnan(got).any(), tag
        assert np.array_equal(got, want), (tag, np.flatnonzero(got != want)[:8])
        assert self.eng.chain_carry() == (2, True), tag

    def full(self, audio, chunk, tag):
        pcm = self.take(audio, np.arange(self.n), chunk)
        self.same(self.eng.update(pcm), self.ref.update(pcm), tag)

    def subset(self, audio, chunk, tag):
        ids = self.rng.permutation(self.n)[:int(self.rng.integers(1, self.n_sub + 1))]
        pcm = self.take(audio, ids, chunk)
        self.same(self.eng.update_subset(ids, pcm), self.ref.update_subset(ids, pcm), tag)

    def alternate(self, audio, n_calls, chunks, tag, first=0):
        for u in range(first, first + n_calls):
            chunk = int(chunks[int(self.rng.integers(0, len(chunks)))])
            (self.subset if u % 2 else self.full)(audio, chunk, (tag, u, chunk))

    def close(self):
        for x, y in zip(self.ref.stream_state(), self.eng.stream_state()):
            assert np.array_equal(x, y)
        assert np.array_equal(self.ref.get_vectors(), self.eng.get_vectors())
        self.ref.close(); self.eng.close()


@pytest.mark.parametrize('front', FRONTS)
@pytest.mark.parametrize('n', [33, 70])
def test_the_reader_changes_place(n, front):
    """150 calls, a full update (one workgroup per tile) and a sparse subset (two per tile, the streams of a tile drawn from all
    over the engine) taking turns, chunks drawn from CHUNKS: what one call stored is read by other workgroups of the next.  33
    streams: one lane into a third tile; 70: four tiles and six streams.  Calls that make 0, 1 and 2 rows visible follow each
    other; a call with none reads the stored chain of age T, one launch after it was written, without stepping it"""
    p = Pair(n, front, 20261021 + n)
    audio = _audio(n, 150 * max(CHUNKS))
    p.alternate(audio, 150, CHUNKS, 'turns')
    assert p.rows == {0, 1, 2}
    assert p.eng.chain_skip() == 0
    p.close()


@pytest.mark.parametrize('front', FRONTS)
def test_the_rebuild_in_between(front):
    """a set_weights and a masked clear in the middle of such a sequence: gru_chains_rebuild_kernel then writes every cell and the
    next chain launch reads them.  Then 1024 samples held for more than N_SKIP calls, so that the instantiation that leaves chains
    out is the one that stores, subsets included; then one call with another chunk (a rebuild again) and on"""
    n = 33
    p = Pair(n, front, 7)
    audio = _audio(n, (120 + N_SKIP + 60) * max(CHUNKS))
    p.alternate(audio, 40, CHUNKS, 'before')
    w2 = _weights(seed=7)
    p.ref.set_weights(w2); p.eng.set_weights(w2)
    assert p.eng.chain_carry() == (2, False)
    p.alternate(audio, 30, CHUNKS, 'new weights', first=1)        # (the first call behind the rebuild is a sparse subset)
    mask = np.arange(n) % 2 == 1
    p.ref.clear(mask); p.eng.clear(mask)
    assert p.eng.chain_carry() == (2, False)
    p.alternate(audio, 30, CHUNKS, 'cleared')                     # (... a full update)
    for u in range(N_SKIP + 2):
        p.full(audio, 1024, ('held', u))
    assert p.eng.chain_skip() == 1024
    for u in range(20):
        (p.subset if u % 2 else p.full)(audio, 1024, ('held turns', u))
        assert p.eng.chain_skip() == 1024
    p.full(audio, 1088, 'left')
    assert p.eng.chain_skip() == 0
    p.alternate(audio, 20, CHUNKS, 'after', first=1)
    p.close()


@pytest.mark.parametrize('front', FRONTS)
def test_an_output_in_pinned_host_memory(front):
    """the update's output pointer lies in memory from host_array (what the async ring and a direct gather hand the launch): the
    values the host reads after a synchronize are the reference's, for full updates and for subsets"""
    import torch
    n = 17
    p = Pair(n, front, 3)
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    audio = _audio(n, 60 * max(CHUNKS))
    out = p.eng.host_array((n,), np.float32)
    for u in range(60):
        chunk = int(CHUNKS[int(p.rng.integers(0, len(CHUNKS)))])
        out[:] = np.nan
        if u % 2:
            ids = p.rng.permutation(n)[:int(p.rng.integers(1, p.n_sub + 1))]
            pcm = p.take(audio, ids, chunk)
            want = p.ref.update_subset(ids, pcm)
            d_ids, d_pcm = torch.from_numpy(ids.astype(np.int32)).to(dev), torch.from_numpy(pcm).to(dev)
            p.eng.update_subset_device(d_ids.data_ptr(), ids.size, d_pcm.data_ptr(), chunk, out.ctypes.data, st)
        else:
            ids = np.arange(n)
            pcm = p.take(audio, ids, chunk)
            want = p.ref.update(pcm)
            d_pcm = torch.from_numpy(pcm).to(dev)
            p.eng.update_device(d_pcm.data_ptr(), chunk, out.ctypes.data, st)
        torch.cuda.synchronize()
        p.same(out[:ids.size].copy(), want, (u, chunk))
        assert np.isnan(out[ids.size:]).all()
    del out
    p.close()
