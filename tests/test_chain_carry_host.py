"""
CPU only: the index algebra of the carried window chains (csrc/gru_chain_device.h), as a plain-Python model, and the knob's
declaration and binding.

The model restates the record arithmetic of gru_ke_resolve / mfcc_book_tile (q, kc, ke per stream) and the schedule of
gru_tile_chains: chain of start row s lives in slot s & 31, an update that makes k rows visible advances the chain of
post-update age a by min(a, k) steps over the rows ke_post - min(a, k) .. ke_post - 1, chains of age a <= k are born from
nothing.  A "state" here is the list of rows a chain has consumed; the feature ring is modelled as 32 slots that hold row
indices, overwritten as the frames are computed.  What is asserted at every update of every stream:

  * the chain headed (age T) has consumed exactly the rows ke - T .. ke - 1, in order;
  * every row a step consumes is still in its ring slot when it is read;
  * no live chain's slot is overwritten (a slot is reused only by the chain that starts 32 rows later);
  * the stamp (chain_ke) equals the record's emitted count before the update.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from mycroft_precise_amd import _lib

T, SLOTS, HOP, WINDOW, FRAME = 29, 32, 800, 1600, 512        # stock ListenerParams: n_features, ring, hop, window, min(window, n_fft)
MAX_ROWS = 2                                                 # kChainMaxRows


class Stream:
    """One stream's record (mfcc_book_tile), its ring slots and its carried chains."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.q, self.kc, self.ke = 0, 0, 0
        self.ring = [None] * SLOTS           # row index held by each slot (None: the zero rows of a cleared stream)
        self.chains = [None] * SLOTS         # per slot: (start, [rows consumed])
        self.stamp = None

    def row(self, r):
        """the ring row a step reads for row index r (rows before the stream's start are zero rows)"""
        if r < 0:
            assert self.ring[r % SLOTS] is None, 'a zero row was overwritten while a window still reads it'
            return r
        assert self.ring[r % SLOTS] == r, 'row %d is no longer in its slot' % r
        return r

    def predict(self, chunk):
        """gru_ke_resolve with predict_ke, and the record after the update"""
        avail = self.q + chunk
        nnew = 1 + (avail - FRAME) // HOP if avail >= FRAME else 0
        qn = avail - nnew * HOP
        m = qn + HOP * (self.kc + nnew - self.ke)
        ke = self.ke + (1 + (m - WINDOW) // HOP if m >= WINDOW else 0)
        return ke, (qn, self.kc + nnew, ke), nnew

    def rebuild(self):
        """gru_tile_chains_rebuild: chain of age a = rows ke - a .. ke - 1"""
        self.chains = [None] * SLOTS
        for a in range(1, T + 1):
            s = self.ke - a
            self.chains[s % SLOTS] = (s, [self.row(s + i) for i in range(a)])
        self.stamp = self.ke

    def window_rows(self, ke):
        return [self.row(r) for r in range(ke - T, ke)]

    def update(self, chunk, carried, kmax_of_wave=None):
        """One fused update of this stream.  Returns the rows the headed window consumed."""
        ke_pre = self.ke
        ke_post, rec, nnew = self.predict(chunk)
        k = ke_post - ke_pre
        assert 0 <= k <= MAX_ROWS
        head = None
        if carried:
            assert self.stamp == ke_pre, 'the chains are not current to the record'
            kmax = k if kmax_of_wave is None else kmax_of_wave
            assert kmax >= k
            for a in range(1, T + 1):
                slot = (ke_post - a) % SLOTS
                if a <= k:                                   # born in this update
                    old = self.chains[slot]
                    assert old is None or old[0] == ke_post - a - SLOTS or ke_post - old[0] > T, 'a live chain is overwritten'
                    start, rows = ke_post - a, []
                else:
                    start, rows = self.chains[slot]
                    assert start == ke_post - a
                for i in range(kmax):                        # the wave's trip count; the lane keeps what is its own
                    if i < k and k <= a + i:
                        rows = rows + [self.row(ke_pre + i)]
                self.chains[slot] = (start, rows)
                if a == T:
                    head = rows
            self.stamp = ke_post
        else:
            head = self.window_rows(ke_post)
        # the frame role and the books: the rows this update computes land in the ring (visible in a LATER update)
        for r in range(self.kc, self.kc + nnew):
            assert r >= ke_post, 'a frame computed by an update became visible in it'
            self.ring[r % SLOTS] = r
        self.q, self.kc, self.ke = rec
        return head


def check_head(st, head):
    assert head == list(range(st.ke - T, st.ke)), (head, st.ke)


@pytest.mark.parametrize('chunks', [[1024] * 140, [800] * 120, [160] * 600, [1088] * 130, None], ids=['1024', '800', '160', '1088', 'mix'])
@pytest.mark.parametrize('enter_after', [0, 1, 7, 24])
def test_headed_chain_has_consumed_exactly_its_window(chunks, enter_after):
    rng = np.random.default_rng(5 + enter_after)
    if chunks is None:
        chunks = [int(c) for c in 2 * rng.integers(80, 545, 300)]
    st = Stream()
    seen_k = set()
    for u, c in enumerate(chunks):
        if u == enter_after:
            st.rebuild()
        ke0 = st.ke
        head = st.update(c, carried=u >= enter_after)
        seen_k.add(st.ke - ke0)
        check_head(st, head)
    assert st.ke > 3 * SLOTS                                  # >= 3 ring wraps and chain lifetimes
    assert seen_k <= {0, 1, 2} and len(seen_k) >= 1


def test_k_cycle_of_the_headline_chunk():
    """1024-sample chunks: k alternates between 1 and 2 over a 25-update cycle (32 rows)"""
    st = Stream()
    ks = []
    for _ in range(100):
        ke0 = st.ke
        st.update(1024, carried=False)
        ks.append(st.ke - ke0)
    tail = ks[50:75]
    assert sorted(set(tail)) == [1, 2] and sum(tail) == 32 and tail == ks[75:100]


def test_streams_out_of_phase_subsets_and_clears():
    """16 streams of one tile at private phases and cadences; subset calls advance some of them (the wave's trip count is the
    largest k among ALL lanes of the call, a stream outside the call keeps chains and stamp); a clear invalidates everything
    (the epoch rule) and the chains are rebuilt before the next chain launch."""
    rng = np.random.default_rng(11)
    n = 16
    sts = [Stream() for _ in range(n)]
    for s, st in enumerate(sts):                             # private phases: an odd first chunk each, plain updates
        check_head(st, st.update(int(2 * rng.integers(80, 545)), carried=False))
    valid = False
    for call in range(400):
        chunk = int(2 * rng.integers(80, 545))
        active = [s for s in range(n) if rng.random() < 0.2 + 0.6 * (s % 4) / 3]
        if call % 97 == 50:                                  # a masked clear: every stream's chains count as invalid
            for s in active[::2]:
                sts[s].clear()
            valid = False
            continue
        if not valid:
            for st in sts:
                st.rebuild()
            valid = True
        kmax = max([sts[s].predict(chunk)[0] - sts[s].ke for s in active], default=0)
        idle = [(st.chains[:], st.stamp, st.ke) for st in sts]
        for s in active:
            check_head(sts[s], sts[s].update(chunk, carried=True, kmax_of_wave=kmax))
        for s in set(range(n)) - set(active):
            assert (sts[s].chains, sts[s].stamp, sts[s].ke) == idle[s]
    assert len({st.ke for st in sts}) > n // 2


@pytest.mark.parametrize('nw', [4, 8])
def test_wave_split_covers_every_age_once(nw):
    """wave w of the nw that share a tile (4, or 8 for sparse subset calls) takes the ages a = w (mod nw), two at a time; the wave
    T % nw holds the window"""
    for t in range(1, T + 1):
        ages = []
        for wave in range(nw):
            a0 = wave if wave else nw
            while a0 <= t:
                ages.append(a0)
                if a0 + nw <= t:
                    ages.append(a0 + nw)
                if t in (a0, a0 + nw):
                    assert wave == t % nw
                a0 += 2 * nw
        assert sorted(ages) == list(range(1, t + 1))


def test_chain_state_layout_is_a_bijection():
    """chain_cell: [tile][32 slots][5 rho][64 lanes], lane = 16 g + (stream & 15)"""
    n_padded = 48
    cells = set()
    for sid in range(n_padded):
        for slot in range(SLOTS):
            for g in range(4):
                for rho in range(5):
                    cells.add((((sid >> 4) * SLOTS + slot) * 5) * 64 + g * 16 + (sid & 15) + rho * 64)
    assert len(cells) == n_padded * SLOTS * 20 and max(cells) == n_padded // 16 * SLOTS * 5 * 64 - 1


# ---- the knob: declared, exported, bound ------------------------------------------------------------------------------------
def test_knob_is_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'precise_engine.h')).read()
    assert re.search(r'^int pe_set_chain_carry\(pe_engine\* e, int32_t mode\);', header, re.M)
    assert re.search(r'^int pe_get_chain_carry\(const pe_engine\* e, int32_t\* mode, int32_t\* active\);', header, re.M)
    assert re.search(r'#define PE_ABI_VERSION 8\b', header)                      # additive
    assert _lib.EXPORTS['pe_set_chain_carry'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32])
    assert _lib.EXPORTS['pe_get_chain_carry'][1][1:] == [ctypes.POINTER(ctypes.c_int32)] * 2
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'pe_set_chain_carry') and hasattr(raw, 'pe_get_chain_carry')
    assert callable(_lib.HipEngine.set_chain_carry) and callable(_lib.HipEngine.chain_carry)
    lib = _lib.load()
    assert lib.pe_set_chain_carry(None, 1) != 0                                 # a null engine is an error, not a crash
    assert lib.pe_get_chain_carry(None, None, None) != 0
