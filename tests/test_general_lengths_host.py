"""CPU: the table of tests/test_general_lengths.py reaches every transform instantiation of the general front end, and its
inputs are well conditioned in float32 -- so a float32 failure on the GPU is the kernel's, not the input's.
(What pe_create refuses -- 12, 1025, 1500, 4096 -- is tests/test_abi.py's.)"""
import numpy as np
import pytest

import general_lengths_common as G
from oracle import listener as ol
from oracle import sonopy_restated as sr

TOL_FEAT32 = 2e-5       # tests/test_gpu_parity.py: float32 rounding of |feature| <= 40


def test_table_reaches_every_instantiation_the_launchers_dispatch():
    hit = {}
    for kw in G.LENGTHS:
        hit.setdefault(G.instantiation(kw['n_fft']), []).append(kw['n_fft'])
    assert sorted(hit) == sorted(G.DISPATCHED) and len(G.DISPATCHED) == 11
    for key, sets in G.TABLE.items():                   # ... and every set sits in the row the table gives it
        assert [G.instantiation(kw['n_fft']) for kw in sets] == [key] * len(sets), key
    # every length the engine serves lands on a dispatched instantiation
    served = [n for n in range(16, 2049) if G.is_pow2(n) or n <= 1024]
    assert {G.instantiation(n) for n in served} == set(G.DISPATCHED)
    assert all(not G.is_pow2(n) for n in (16, 32)) and G.instantiation(16) == G.instantiation(32) == ('blue', 7)


def test_bluestein_boundaries_land_where_the_table_says():
    ns = [kw['n_fft'] for kw in G.LENGTHS]
    for n in G.TIGHTEST:                                # 2 N - 1 three below L: one more sample and the length doubles
        b = G.blue_log2(n)
        assert n in ns and (1 << b) - (2 * n - 1) == 3
        assert G.is_pow2(n + 1) and G.blue_log2(n + 2) == b + 1
    for n in G.LOOSEST:                                 # the first n_fft of its length: 2 N - 1 is one past the length below
        b = G.blue_log2(n)
        assert n in ns and 2 * n - 1 == (1 << (b - 1)) + 1
        assert G.blue_log2(n - 2) == b - 1
    assert [G.blue_log2(n) for n in G.TIGHTEST] == [7, 8, 9, 10, 11]
    assert [G.blue_log2(n) for n in G.LOOSEST] == [8, 9, 10, 11]
    assert G.blue_log2(1024 - 1) == 11 and (1 << 11) >= 2 * 1023 - 1         # the longest Bluestein n_fft fits the longest length


@pytest.mark.parametrize('kw', G.LENGTHS, ids=G.set_id)
def test_float32_restatement_stays_at_float32_rounding_of_the_oracle(kw):
    """every input kind of the GPU test, offline buffers: worst |float32 restatement - float64 oracle| <= TOL_FEAT32"""
    opr = ol.Params(**kw)
    win_hop = (opr.window_samples, opr.hop_samples)
    for kind, audio in G.offline_inputs(kw['n_fft']):
        _, _, want_mels, want = sr.mfcc_spec(audio, opr.sample_rate, win_hop, opr.n_fft, opr.n_filt, opr.n_mfcc, return_parts=True)
        got, got_mels = G.float32_restatement(G.frames_of(audio, *win_hop), opr.n_fft, opr.n_filt, opr.n_mfcc, opr.sample_rate, with_mels=True)
        assert got.shape == want.shape == (1 + (G.N_SAMPLES - win_hop[0]) // win_hop[1], kw['n_mfcc'])
        err, err_mels = float(np.abs(got - want).max()), float(np.abs(got_mels - want_mels).max())
        print('%s %s: features %.3g, mels %.3g' % (G.set_id(kw), kind, err, err_mels))
        assert err <= TOL_FEAT32, (kind, err)
        # (the log-mel rows have no bar of their own here: 80 filters over 257 bins put single-bin filters on the square wave's
        #  spectral nulls, 2.4e-5; the GPU test holds the float32 kernels' rows to 2e-4 and to 8 x this figure)
        assert err_mels <= 2e-4, (kind, err_mels)
