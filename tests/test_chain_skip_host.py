"""CPU: pe_chain_alive_mask (csrc/pe_common.h: ke_step + chain_alive_bits), the predicate a chain launch skips carried chains by,
against a brute-force replay of the streams' bookkeeping.

The replay knows nothing of the formula: it advances one stream's record (q leftover samples, kc computed frames, ke emitted rows)
update by update with the arithmetic of the bookkeeping kernel, notes the emitted count every update ends with -- an update hands
out ONE window, the chain started T rows before that count --, and calls a chain alive iff a later update ends exactly T rows
after its start.  Every comparison is for equality; the only bound is the issue's 0.5 % on the share of dead starts.
"""
import numpy as np
import pytest

from mycroft_precise_amd import _lib
from mycroft_precise_amd import params as P

HOP = P.pr.hop_samples
WINDOW = P.pr.window_samples
FRAME = min(P.pr.window_samples, P.pr.n_fft)
T = P.pr.n_features
CHUNKS = (160, 800, 802, 900, 1024, 1088)
N_HISTORIES, N_UPDATES = 20, 600
# a chain of age 1 still needs T - 1 rows: at most that many hops of samples, and a margin
def _horizon(c):
    return (T * HOP) // c + 8


def _step(q, kc, ke, c):
    """one update of c samples (mfcc_book_tile's arithmetic, restated)"""
    avail = q + c
    nnew = 1 + (avail - FRAME) // HOP if avail >= FRAME else 0
    q = avail - nnew * HOP
    kc += nnew
    held = q + HOP * (kc - ke)
    if held >= WINDOW:
        ke += 1 + (held - WINDOW) // HOP
    return q, kc, ke


def _replay(c, seed):
    """(record before the update, emitted count after it) of every update of a run with chunk c after a random prehistory"""
    rng = np.random.default_rng(seed)
    q = kc = ke = 0
    for chunk in rng.integers(1, 1601, size=int(rng.integers(3, 40))):
        q, kc, ke = _step(q, kc, ke, int(chunk))
    recs, ends = [], []
    for _ in range(N_UPDATES + _horizon(c)):
        recs.append((q, kc, ke))
        q, kc, ke = _step(q, kc, ke, c)
        ends.append(ke)
    return recs, ends


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def test_geometry_is_the_stock_one():
    assert (HOP, WINDOW, FRAME, T) == (800, 1600, 512, 29)


@pytest.mark.parametrize('c', CHUNKS)
def test_mask_agrees_with_the_replay(lib, c):
    born = dead = 0
    for seed in range(N_HISTORIES):
        recs, ends = _replay(c, 1000 * c + seed)
        handed = set(e - T for e in ends)                   # the starts whose window some update of the run hands out
        for u in range(N_UPDATES):
            q, kc, ke = recs[u]
            mask = lib.pe_chain_alive_mask(q, kc, ke, c, HOP, FRAME, WINDOW, T)
            later = set(e - T for e in ends[u + 1:u + 1 + _horizon(c)])
            assert ends[u + _horizon(c)] >= ends[u] + T     # the replay looks far enough ahead for the youngest chain
            want = 1 << T                                   # age T: this update's own window
            for age in range(1, T):
                if ends[u] - age in later:
                    want |= 1 << age
            assert mask == want, (c, seed, u, recs[u], bin(mask), bin(want))
            assert mask >> T == 1 and not mask & 1
            k = ends[u] - ke
            for age in range(1, min(k, T - 1) + 1):         # every start is born once: counted there
                born += 1
                dead += not (mask >> age) & 1
        assert handed                                       # (the set the test is about is not empty)
    assert born > 0
    share = dead / born
    print('chunk %d: %d of %d starts dead = %.4f, 1 - hop / c = %.4f' % (c, dead, born, share, max(0.0, 1 - HOP / c)))
    if c <= HOP:
        assert dead == 0
    else:
        assert abs(share - (1 - HOP / c)) <= 0.005


def test_arguments_out_of_range_give_no_mask(lib):
    ok = (100, 5, 3, 1024, HOP, FRAME, WINDOW, T)
    assert lib.pe_chain_alive_mask(*ok) >> T == 1
    # (q: the bookkeeping leaves frame_len - hop <= q < frame_len: -1 and frame_len - hop are a record's values here, anything below is not)
    assert lib.pe_chain_alive_mask(-1, *ok[1:]) >> T == 1 == lib.pe_chain_alive_mask(FRAME - HOP, *ok[1:]) >> T
    for i, bad in ((0, FRAME - HOP - 1), (0, -HOP), (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (7, 32)):
        args = list(ok)
        args[i] = bad
        assert lib.pe_chain_alive_mask(*args) == 0


def test_getter_is_bound_and_refuses_a_null_engine(lib):
    import ctypes as C
    assert 'pe_get_chain_skip' in _lib.EXPORTS and 'pe_chain_alive_mask' in _lib.EXPORTS
    assert lib.pe_get_chain_skip(None, C.byref(C.c_int32(7))) != 0
    assert _lib.ABI_VERSION == 8 == lib.pe_abi_version()


def test_the_run_lengths_are_written_the_same_everywhere():
    """kChainSkipAfter and kChainEnterAfter (engine.hip) are quoted in the header, in INTEGRATION.md and as N_SKIP / N_ENTER in the
    GPU tests: one place to change, and this test to name the others"""
    import os
    import re
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def text(*parts):
        with open(os.path.join(repo, *parts)) as f:
            return f.read()
    eng = text('mycroft_precise_amd', 'csrc', 'engine.hip')
    skip = int(re.search(r'constexpr int kChainSkipAfter = (\d+);', eng).group(1))
    enter = int(re.search(r'constexpr int kChainEnterAfter = (\d+);', eng).group(1))
    header = re.sub(r'\s+\*?\s*', ' ', text('include', 'precise_engine.h'))
    assert 'after %d eligible update calls in a row the engine builds' % enter in header
    assert 'After %d eligible calls in a row with the same chunk > hop' % skip in header
    assert 'after %d eligible calls in a row with the same chunk' % skip in text('INTEGRATION.md')
    for name in ('test_chain_skip.py', 'test_chain_carry.py'):
        src = text('tests', name)
        assert re.search(r'^N_ENTER = %d\b' % enter, src, flags=re.M), name
    assert re.search(r'^N_SKIP = %d\b' % skip, text('tests', 'test_chain_skip.py'), flags=re.M)
