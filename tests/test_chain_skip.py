"""
Chains that are never handed out (csrc/gru_chain_device.h: ChainArgs::skip; engine.hip: kChainSkipAfter).  Once a caller's chunk
has held for N_SKIP eligible calls, a chain launch neither loads, steps nor stores the carried chains that no update of that
cadence will hand out.  That must change no bit: as in test_chain_carry, the reference of every comparison is the same engine
class with set_chain_carry(0), fed the same chunks, compared with np.array_equal after every update.  No tolerance appears.
Every call also checks that no output is NaN (the stamp cross-check of a chain launch), that the chains stay active, and that
chain_skip() reports what include/precise_engine.h documents; every case ends with equal stream_state().
"""
import numpy as np
import pytest

from mycroft_precise_amd import synth
from mycroft_precise_amd import params as P

pytestmark = pytest.mark.gpu

N_ENTER = 128           # eligible calls in a row before the automatic mode builds its chains (precise_engine.h)
N_SKIP = 128            # eligible calls in a row with one chunk > hop before unneeded chains are left out (precise_engine.h)
HOP = P.pr.hop_samples


def _engine(weights, n, mode, **kw):
    from mycroft_precise_amd._lib import HipEngine
    e = HipEngine(P.pr, weights, n_streams=n, **kw)
    e.set_chain_carry(mode)
    return e


def _weights(seed=42):
    return synth.make_weights(n_in=P.pr.n_mfcc, units=(20,), seed=seed)


def _audio(n, total):
    kinds = ['tone_noise'] * (n - 3) + ['zeros', 'square', 'quiet']
    return np.stack([synth.stream_pcm(s, total, k) for s, k in enumerate(kinds)])


class Pair:
    """the reference engine and the engine under test, fed alike, with the host's rule for chain_skip() restated: the run of
    eligible calls with one chunk since the last call that invalidated the chains"""

    def __init__(self, n, mode=2, weights=None, **kw):
        self.n, self.mode = n, mode
        w = _weights() if weights is None else weights
        self.ref, self.eng = _engine(w, n, 0, **kw), _engine(w, n, mode, **kw)
        self.run, self.run_chunk, self.streak = 0, 0, 0
        self.pos = np.zeros(n, dtype=np.int64)

    def bumped(self):
        """something other than an eligible update moved the streams or changed the network"""
        self.run = self.streak = 0
        assert self.eng.chain_carry()[1] is False and self.eng.chain_skip() == 0

    def expect(self, chunk):
        if chunk != self.run_chunk:
            self.run = 0
        self.run, self.run_chunk = self.run + 1, chunk
        self.streak += 1
        active = self.mode == 2 or self.streak > N_ENTER
        return active, (chunk if active and chunk > HOP and self.run >= N_SKIP else 0)

    def check(self, got, want, chunk, tag):
        assert not np.isnan(got).any(), tag
        assert np.array_equal(got, want), (tag, chunk, np.flatnonzero(got != want)[:8])
        active, skip = self.expect(chunk)
        assert self.eng.chain_carry()[1] == active, tag
        assert self.eng.chain_skip() == skip, (tag, chunk, self.run)
        return skip

    def full(self, audio, chunk, tag=None):
        pcm = np.stack([audio[s, self.pos[s]:self.pos[s] + chunk] for s in range(self.n)])
        self.pos += chunk
        return self.check(self.eng.update(pcm), self.ref.update(pcm), chunk, tag)

    def subset(self, audio, ids, chunk, tag=None):
        ids = np.asarray(ids)
        pcm = np.stack([audio[s, self.pos[s]:self.pos[s] + chunk] for s in ids])
        self.pos[ids] += chunk
        return self.check(self.eng.update_subset(ids, pcm), self.ref.update_subset(ids, pcm), chunk, tag)

    def close(self):
        for x, y in zip(self.ref.stream_state(), self.eng.stream_state()):
            assert np.array_equal(x, y)
        assert np.array_equal(self.ref.get_vectors(), self.eng.get_vectors())
        assert self.ref.chain_skip() == 0
        self.ref.close(); self.eng.close()


SHAPES = [(17, 'f64'), (33, 'f32'), (33, 'f64'), (17, 'f32')]


@pytest.mark.parametrize('mode', [2, 1], ids=['eager', 'auto'])
@pytest.mark.parametrize('chunk', [1024, 1088, 900, 802])
def test_constant_chunks(chunk, mode):
    """N_SKIP + 100 updates of one chunk: at least three wraps of the 32-slot ring with chains left out (100 updates of 802 samples
    emit 100 rows).  Eager: skipping from the N_SKIP-th call on; automatic: from the entry, one call later"""
    n, front = SHAPES[([1024, 1088, 900, 802].index(chunk) + (mode == 1)) % 4]
    p = Pair(n, mode, mfcc_precision=front)
    audio = _audio(n, (N_SKIP + 100) * chunk)
    seen = [p.full(audio, chunk, u) for u in range(N_SKIP + 100)]
    first = N_SKIP - 1 if mode == 2 else N_ENTER
    assert seen == [0] * first + [chunk] * (N_SKIP + 100 - first)
    p.close()


@pytest.mark.parametrize('chunk, n_up', [(800, 150), (160, 400)])
def test_chunks_of_at_most_a_hop_never_engage(chunk, n_up):
    p = Pair(17)
    audio = _audio(17, n_up * chunk)
    assert not any(p.full(audio, chunk, u) for u in range(n_up))
    p.close()


def test_leaving_a_cadence():
    """1024 x n, then 1000, then 1024 x n, then a random mix: equal and active on every call; chain_skip() falls to 0 at the call
    with another chunk (which rebuilds every chain first) and comes back only after a full run"""
    n = 33
    mix = [int(c) for c in 2 * np.random.default_rng(5).integers(80, 545, 70)]
    chunks = [1024] * (N_SKIP + 20) + [1000] + [1024] * (N_SKIP + 20) + mix
    p = Pair(n)
    audio = _audio(n, sum(chunks))
    seen = [p.full(audio, c, u) for u, c in enumerate(chunks)]
    assert seen[N_SKIP + 19] == 1024 and seen[N_SKIP + 20] == 0 and seen[2 * N_SKIP + 19] == 0 and seen[2 * N_SKIP + 20] == 1024
    assert not any(seen[2 * N_SKIP + 41:])
    p.close()


def test_leaving_at_every_phase_of_the_cycle():
    """the cadence of 1024 samples is left -- one call of 1056 -- at each of the 25 positions of a stream inside the 25-update
    cycle of that chunk (position inside the hop: a multiple of 32 samples, 1024 moves it by 7 of them, 1056 by 8), on one pair
    of engines: N_SKIP + a few updates of 1024 in front of every change"""
    n = 17
    p = Pair(n)
    plan, phase, todo = [], 0, list(range(25))
    while todo:
        target = todo.pop(0)
        more = next(m for m in range(N_SKIP, N_SKIP + 25) if (phase + 7 * m) % 25 == target)
        plan.append((more, target))
        phase = (target + 8) % 25
    audio = _audio(n, sum(m for m, _ in plan) * 1024 + 25 * 1056 + 40 * 1024)
    left_at = set()
    for more, target in plan:
        seen = [p.full(audio, 1024, (target, u)) for u in range(more)]
        assert seen == [0] * (N_SKIP - 1) + [1024] * (more - N_SKIP + 1)
        left_at.add(int(p.pos[0] % HOP) // 32)
        assert p.full(audio, 1056, target) == 0
    assert left_at == set(range(25))
    for u in range(40):
        assert p.full(audio, 1024, u) == 0
    p.close()


@pytest.mark.parametrize('n', [33, 64])
def test_half_tile_subsets_out_of_phase(n):
    """n streams at private phases -- 33: two tiles and one lane of a third; 64: four full tiles, a cadence of its own for every
    stream as in test_chain_carry.test_half_tiles_at_other_cadences --; every call names a random subset (half of every tile
    takes part in most calls, the other half in few), every tenth call is a full update.  The lanes of a tile differ in emitted count, in k and in which of their chains are dead: a chain is
    left out only where it is dead for the whole tile.  A masked clear and a set_weights in the middle invalidate the
    chains as they always did; skipping comes back after a full run"""
    rng = np.random.default_rng(20261020)
    p = Pair(n)
    n_calls = 3 * N_SKIP + 120
    audio = _audio(n, (n_calls + 4) * 1024 + 2000)
    first = 2 * rng.integers(80, 545, n)
    for length in np.unique(first):
        p.subset(audio, np.flatnonzero(first == length), int(length), ('phase', int(length)))
    cadence = np.where(np.arange(n) % 16 < 8, 0.85, rng.choice([0.2, 0.35, 0.5], n))
    if n == 64:
        cadence = cadence * rng.uniform(0.9, 1.1, n)              # 64 different cadences
        assert len(np.unique(cadence)) == 64
    seen = []
    for call in range(n_calls):
        if call == N_SKIP + 60:
            mask = np.arange(n) % 2 == 1
            p.ref.clear(mask); p.eng.clear(mask)
            p.bumped()
        if call == 2 * N_SKIP + 90:
            w2 = _weights(seed=7)
            p.ref.set_weights(w2); p.eng.set_weights(w2)
            p.bumped()
        if call % 10 == 9:
            seen.append(p.full(audio, 1024, call))
            continue
        active = np.flatnonzero(rng.random(n) < cadence)
        rng.shuffle(active)
        if active.size == 0:
            active = np.array([int(rng.integers(0, n))])
        seen.append(p.subset(audio, active, 1024, call))
    on = [i for i, s in enumerate(seen) if s]
    assert on == (list(range(N_SKIP - 1, N_SKIP + 60)) + list(range(2 * N_SKIP + 59, 2 * N_SKIP + 90))
                  + list(range(3 * N_SKIP + 89, n_calls)))
    assert len(np.unique(p.pos % HOP)) > n // 2
    p.close()


def test_quarter_subset_while_the_others_idle():
    """skipping on after N_SKIP full updates; then ids = 0, 4, 8, ... advance alone for 60 calls (a sparse subset: eight waves per
    tile, two workgroups, both of which must find the same mask), then full updates with every stream where IT is"""
    n = 33
    p = Pair(n)
    audio = _audio(n, (N_SKIP + 140) * 1024)
    for u in range(N_SKIP + 10):
        p.full(audio, 1024, u)
    assert p.eng.chain_skip() == 1024
    ids = np.arange(0, n, 4)
    for u in range(60):
        assert p.subset(audio, ids, 1024, u) == 1024
    for u in range(60):
        assert p.full(audio, 1024, u) == 1024
    assert len(np.unique(p.pos)) == 2
    p.close()


def test_every_entry_point():
    """update, update_device, update_device(keep=True) over two alternating slabs, update_subset[_device], update_async / wait and
    update_subset_async / wait (the call the reference's runner maps to), interleaved on one engine while chains are being left
    out"""
    import torch
    n, n_up = 33, N_SKIP + 80
    rng = np.random.default_rng(4)
    p = Pair(n)
    ref, eng = p.ref, p.eng
    audio = _audio(n, n_up * 1024).reshape(n, n_up, 1024)
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    slabs = [torch.zeros((n, 1024), dtype=torch.int16, device=dev) for _ in range(2)]
    out = torch.zeros(n, device=dev)
    styles = ['host', 'device', 'keep', 'keep', 'subset', 'subset_device', 'async', 'subset_async']
    seen = set()
    for u in range(n_up):
        pcm = np.ascontiguousarray(audio[:, u])
        want = ref.update(pcm)
        style = styles[int(rng.integers(0, len(styles)))]
        if u >= N_SKIP:
            seen.add(style)
        if style == 'host':
            got = eng.update(pcm)
        elif style in ('device', 'keep'):
            slab = slabs[u % 2]
            slab.copy_(torch.from_numpy(pcm))
            eng.update_device(slab.data_ptr(), 1024, out.data_ptr(), st, keep=(style == 'keep'))
            got = out.cpu().numpy()
        elif style == 'subset':
            perm = rng.permutation(n)
            got = np.empty(n, np.float32)
            got[perm] = eng.update_subset(perm, pcm[perm])
        elif style == 'subset_device':
            perm = rng.permutation(n)
            ids = torch.from_numpy(perm.astype(np.int32)).to(dev)
            rows = torch.from_numpy(np.ascontiguousarray(pcm[perm])).to(dev)
            osub = torch.zeros(n, device=dev)
            eng.update_subset_device(ids.data_ptr(), n, rows.data_ptr(), 1024, osub.data_ptr(), st)
            got = np.empty(n, np.float32)
            got[perm] = osub.cpu().numpy()
        elif style == 'subset_async':
            perm = rng.permutation(n)
            res = eng.update_subset_async(perm, pcm[perm])
            eng.wait()
            got = np.empty(n, np.float32)
            got[perm] = res
        else:
            res = eng.update_async(pcm)
            eng.wait()
            got = res
        assert p.check(got, want, 1024, (u, style)) == (1024 if u >= N_SKIP - 1 else 0)
    assert seen == set(styles)
    p.close()
