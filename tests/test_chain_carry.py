"""
Carried window chains (csrc/gru_chain_device.h; pe_set_chain_carry): an engine that advances the GRU chains of every live
window start by the rows an update makes visible must give, BIT FOR BIT, what the same engine gives when it runs every window
again from h = 0.  The reference of every comparison here is the same class with set_chain_carry(0), fed the same chunks;
no tolerance appears except in the one oracle check at the end (and there it is the stock float32 guard of test_gpu_parity).
"""
import numpy as np
import pytest

from mycroft_precise_amd import synth
from mycroft_precise_amd import params as P
from oracle import listener as ol
from test_gpu_parity import GUARD_RAW

pytestmark = pytest.mark.gpu

N_ENTER = 128           # eligible calls in a row before the automatic mode builds its chains (precise_engine.h)


def _engine(weights, n, mode, **kw):
    from mycroft_precise_amd._lib import HipEngine
    e = HipEngine(P.pr, weights, n_streams=n, **kw)
    e.set_chain_carry(mode)
    return e


def _weights(units=20, seed=42):
    return synth.make_weights(n_in=P.pr.n_mfcc, units=(units,), seed=seed)


def _audio(n, total):
    """int16 [n][total]: tones in noise, and -- the last three streams -- silence, a full-scale square wave, a quiet stream"""
    kinds = ['tone_noise'] * (n - 3) + ['zeros', 'square', 'quiet']
    return np.stack([synth.stream_pcm(s, total, k) for s, k in enumerate(kinds)])


def _chunks(name, n_updates, seed=0):
    if name == 'mix':
        return [int(c) for c in 2 * np.random.default_rng(seed).integers(80, 545, n_updates)]         # even, 160 .. 1088
    return [int(name)] * n_updates


def _run_pair(ref, eng, audio, chunks, expect_active_from=None):
    """the same chunks through both engines; outputs equal after every update"""
    pos = 0
    for u, c in enumerate(chunks):
        pcm = audio[:, pos:pos + c]
        pos += c
        want, got = ref.update(pcm), eng.update(pcm)
        assert np.array_equal(got, want), (u, c, np.flatnonzero(got != want)[:8])
        if expect_active_from is not None:
            assert eng.chain_carry()[1] == (u >= expect_active_from), u
    return pos


SEQS = {'1024': 125, '800': 110, '160': 560, '1088': 125, 'mix': 180}         # updates: >= 100 after entry, >= 3 ring wraps


@pytest.mark.parametrize('front', ['f64', 'f32'])
@pytest.mark.parametrize('mode', [2, 1], ids=['eager', 'auto'])
@pytest.mark.parametrize('seq', list(SEQS))
def test_chunk_sequences(seq, mode, front):
    """constant 1024 (k alternates 1 / 2), 800 (k = 1), 160 (mostly k = 0), 1088 (the largest fusable chunk) and a random mix, both
    front ends (the _nopk twin), eager entry and the automatic one after N_ENTER eligible calls; 17 streams (a second tile
    with 15 padded lanes)"""
    n = 17
    w = _weights()
    chunks = _chunks(seq, SEQS[seq] + (N_ENTER if mode == 1 else 0), seed=3)
    audio = _audio(n, sum(chunks))
    ref, eng = _engine(w, n, 0, mfcc_precision=front), _engine(w, n, mode, mfcc_precision=front)
    assert eng.chain_carry() == (mode, False) and ref.chain_carry() == (0, False)
    _run_pair(ref, eng, audio, chunks, expect_active_from=0 if mode == 2 else N_ENTER)
    assert not ref.chain_carry()[1]
    for x, y in zip(ref.stream_state(), eng.stream_state()):
        assert np.array_equal(x, y)
    assert ref.info().device_bytes < eng.info().device_bytes       # the chain state is allocated at the first entry only
    ref.close(); eng.close()


@pytest.mark.parametrize('n', [16, 17, 48])
@pytest.mark.parametrize('units', [17, 18, 19, 20])
def test_units_and_stream_counts(units, n):
    w = _weights(units, seed=100 + units)
    chunks = _chunks('mix', 130, seed=units + n)
    audio = _audio(n, sum(chunks))
    ref, eng = _engine(w, n, 0), _engine(w, n, 2)
    _run_pair(ref, eng, audio, chunks, expect_active_from=0)
    ref.close(); eng.close()


def test_entry_at_every_phase_of_the_cycle():
    """the rebuild after 0, 1, ... 24 plain updates of 1024 samples (the 25-update cycle of k), then 40 carried updates; one
    reference run shared by all"""
    n, n_up = 17, 24 + 40
    w = _weights()
    audio = _audio(n, n_up * 1024).reshape(n, n_up, 1024)
    ref = _engine(w, n, 0)
    want = [ref.update(audio[:, u]) for u in range(n_up)]
    ref.close()
    for phase in range(25):
        eng = _engine(w, n, 0)
        for u in range(phase + 40):
            if u == phase:
                eng.set_chain_carry(2)
            assert np.array_equal(eng.update(audio[:, u]), want[u]), (phase, u)
            assert eng.chain_carry()[1] == (u >= phase)
        eng.close()


def test_masked_clear_desynchronises_a_tile():
    """streams 1, 3, 5, ... cleared in the middle: the tile's lanes are then at different emitted counts and different k"""
    n = 48
    w = _weights()
    chunks = _chunks('1024', 40) + _chunks('mix', 120, seed=9)
    audio = _audio(n, sum(chunks) + 600)
    ref, eng = _engine(w, n, 0), _engine(w, n, 2)
    pos = _run_pair(ref, eng, audio, chunks[:30])
    odd = np.arange(1, n, 2)
    half = np.stack([audio[s, pos:pos + 600] for s in odd])        # the odd streams alone first: another phase inside the chunk cycle
    assert np.array_equal(eng.update_subset(odd, half), ref.update_subset(odd, half))
    mask = (np.arange(n) % 2 == 1)
    ref.clear(mask); eng.clear(mask)
    assert not eng.chain_carry()[1]                                # a masked clear invalidates every stream's chains
    _run_pair(ref, eng, audio[:, pos:], chunks[30:], expect_active_from=0)
    for x, y in zip(ref.stream_state(), eng.stream_state()):
        assert np.array_equal(x, y)
    ref.close(); eng.close()


def test_half_tiles_at_other_cadences():
    """64 streams, every call a random subset at a per-stream cadence and a random fusable chunk (modelled on
    test_streams_advance_independently): inside a tile the lanes differ in emitted count, k and whether they take part"""
    n, n_calls = 64, 170
    w = _weights()
    rng = np.random.default_rng(20261020)
    audio = _audio(n, n_calls * 1088 + 2000)
    ref, eng = _engine(w, n, 0), _engine(w, n, 2)
    pos = np.zeros(n, dtype=np.int64)
    first = 2 * rng.integers(80, 545, n)                           # private phases: one first chunk length per stream
    for length in np.unique(first):
        ids = np.flatnonzero(first == length)
        pcm = np.stack([audio[s, :length] for s in ids])
        assert np.array_equal(eng.update_subset(ids, pcm), ref.update_subset(ids, pcm))
        pos[ids] = length
    cadence = np.where(np.arange(n) % 16 < 8, 0.85, rng.choice([0.2, 0.35, 0.5], n))       # half of every tile at another cadence
    n_active = 0
    for call in range(n_calls):
        chunk = int(2 * rng.integers(80, 545))
        active = np.flatnonzero(rng.random(n) < cadence)
        rng.shuffle(active)
        if active.size == 0:
            continue
        pcm = np.stack([audio[s, pos[s]:pos[s] + chunk] for s in active])
        want, got = ref.update_subset(active, pcm), eng.update_subset(active, pcm)
        assert np.array_equal(got, want), (call, chunk)
        assert eng.chain_carry()[1]
        pos[active] += chunk
        n_active += 1
    assert n_active >= 150 and len(np.unique(pos)) > n // 2
    for x, y in zip(ref.stream_state(), eng.stream_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(ref.get_vectors(), eng.get_vectors())
    ref.close(); eng.close()


def test_quarter_subset_while_the_others_idle():
    """ids = 0, 4, 8, ... advance for 60 calls while the other streams idle (their chains and stamps stay valid), then full
    updates again"""
    n = 48
    w = _weights()
    audio = _audio(n, 200 * 1024)
    ref, eng = _engine(w, n, 0), _engine(w, n, 2)
    pos = _run_pair(ref, eng, audio, _chunks('1024', 30))
    ids = np.arange(0, n, 4)
    p4 = pos
    for u in range(60):
        pcm = audio[ids, p4:p4 + 1024]
        p4 += 1024
        assert np.array_equal(eng.update_subset(ids, pcm), ref.update_subset(ids, pcm)), u
        assert eng.chain_carry()[1]
    for u in range(60):                                            # full updates: every stream from where IT is
        pcm = np.stack([audio[s, (p4 if s % 4 == 0 else pos) + u * 1024:][:1024] for s in range(n)])
        assert np.array_equal(eng.update(pcm), ref.update(pcm)), u
        assert eng.chain_carry()[1]
    ref.close(); eng.close()


def test_every_entry_point():
    """update, update_device, update_device(keep=True) over two alternating slabs, update_subset[_device], update_async / wait --
    interleaved on one engine; the chains stay valid across all of them"""
    import torch
    n, n_up = 48, 110
    w = _weights()
    rng = np.random.default_rng(4)
    audio = _audio(n, n_up * 1024).reshape(n, n_up, 1024)
    ref, eng = _engine(w, n, 0), _engine(w, n, 2)
    dev = torch.device('cuda', 0)
    st = torch.cuda.current_stream().cuda_stream
    slabs = [torch.zeros((n, 1024), dtype=torch.int16, device=dev) for _ in range(2)]
    out = torch.zeros(n, device=dev)
    styles = ['host', 'device', 'keep', 'keep', 'subset', 'subset_device', 'async']
    seen = set()
    for u in range(n_up):
        pcm = np.ascontiguousarray(audio[:, u])
        want = ref.update(pcm)
        style = styles[int(rng.integers(0, len(styles)))] if u >= len(styles) else styles[u]
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
        else:
            res = eng.update_async(pcm)
            eng.wait()
            got = res
        assert np.array_equal(got, want), (u, style)
        assert eng.chain_carry()[1], (u, style)
    assert seen == set(styles)
    ref.close(); eng.close()


def test_leaving_and_reentering():
    """set_weights, set_vectors, clear(), a 2048-sample chunk (not fusable): after each the chains are invalid, outputs stay
    equal, and the engine (automatic mode, the real N) is active again after N_ENTER eligible calls.  update_many comes last:
    it needs pe_reserve_updates, which re-lays the feature ring with more than 32 slots and restarts the streams -- such an
    engine is no longer eligible, so it stays inactive (and equal) from there on."""
    n = 17
    w, w2 = _weights(), _weights(seed=7)
    audio = _audio(n, 100 * 1024)                                  # (fed round and round: both engines hear the same)
    ref, eng = _engine(w, n, 0), _engine(w, n, 1)
    state = {'pos': 0}

    def step(chunk=1024):
        if state['pos'] + chunk > audio.shape[1]:
            state['pos'] = 0
        pcm = audio[:, state['pos']:state['pos'] + chunk]
        state['pos'] += chunk
        want, got = ref.update(pcm), eng.update(pcm)
        assert np.array_equal(got, want), state['pos']

    def reenter():
        assert not eng.chain_carry()[1]
        for i in range(N_ENTER):
            step()
            assert not eng.chain_carry()[1], i
        for i in range(35):
            step()
            assert eng.chain_carry()[1], i

    reenter()
    ref.set_weights(w2); eng.set_weights(w2)
    reenter()
    feats = np.random.default_rng(1).standard_normal((n, P.pr.n_features, P.pr.n_mfcc)).astype(np.float32)
    ref.set_vectors(feats); eng.set_vectors(feats)
    reenter()
    ref.clear(); eng.clear()
    reenter()
    step(2048)
    reenter()
    eng.set_chain_carry(0)
    assert eng.chain_carry() == (0, False)
    for i in range(20):
        step()
    assert not eng.chain_carry()[1]
    eng.set_chain_carry(1)
    reenter()
    for e in (ref, eng):
        e.reserve_updates(2, 1024)
    assert not eng.chain_carry()[1]
    many = np.ascontiguousarray(audio[:, :2048].reshape(n, 2, 1024).transpose(1, 0, 2))
    assert np.array_equal(eng.update_many(many), ref.update_many(many))
    for i in range(N_ENTER + 10):
        step()
        assert not eng.chain_carry()[1]
    ref.close(); eng.close()


@pytest.mark.parametrize('case', ['8208_streams', 'two_models', 'use_delta', 'bf16', 'classic_tiling'])
def test_not_eligible_stays_inactive_and_equal(case):
    import warnings
    from mycroft_precise_amd._lib import HipEngine
    n, kw, pr, w = 17, {}, P.pr, _weights()
    n_up = 24
    if case == '8208_streams':
        n, n_up = 8208, 6
    elif case == 'two_models':
        w = [_weights(), _weights(seed=8)]
    elif case == 'use_delta':
        pr = P.pr.copy()
        pr.__dict__['use_delta'] = True
        w = synth.make_weights(n_in=2 * pr.n_mfcc, units=(20,), seed=13)
    elif case == 'bf16':
        kw = dict(gru_precision='bf16')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ref, eng = HipEngine(pr, w, n_streams=n, **kw), HipEngine(pr, w, n_streams=n, **kw)
    ref.set_chain_carry(0); eng.set_chain_carry(2)
    if case == 'classic_tiling':
        ref.set_gru_tiling(0); eng.set_gru_tiling(0)
    base = _audio(min(n, 48), n_up * 1024)
    audio = np.tile(base, (-(-n // base.shape[0]), 1))[:n]
    for u in range(n_up):
        pcm = audio[:, u * 1024:(u + 1) * 1024]
        assert np.array_equal(eng.update(pcm), ref.update(pcm)), u
        assert eng.chain_carry() == (2, False)
    assert ref.info().device_bytes == eng.info().device_bytes      # never entered: nothing allocated
    ref.close(); eng.close()


@pytest.mark.parametrize('n', [4096, 4112, 8192])
def test_launch_geometry(n):
    """one tile and two frame workgroups per compute unit, a ragged tile count, two tiles and four frame workgroups per compute
    unit: 60 updates each, bit-equality only"""
    import torch
    w = _weights()
    dev = torch.device('cuda', 0)
    base = synth.batch_pcm(64, 20)                                  # [20][64][1024]
    pcm = torch.from_numpy(np.ascontiguousarray(np.tile(base, (1, -(-n // 64), 1))[:, :n])).to(dev)
    ref, eng = _engine(w, n, 0), _engine(w, n, 2)
    oa, ob = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for u in range(60):
        ref.update_device(pcm[u % 20].data_ptr(), 1024, oa.data_ptr(), st)
        eng.update_device(pcm[u % 20].data_ptr(), 1024, ob.data_ptr(), st)
        assert torch.equal(oa, ob), u
    assert eng.chain_carry() == (2, True) and not bool(torch.isnan(ob).any())
    ref.close(); eng.close()


def test_against_the_oracle():
    """48 streams, 120 updates against oracle.listener.BatchedOracle at the guard of the stock float32 parity tests; no NaN
    anywhere: the chain_ke cross-check never fires"""
    n, n_up = 48, 120
    w = _weights()
    audio = _audio(n, n_up * 1024).reshape(n, n_up, 1024)
    eng = _engine(w, n, 2)
    ref = ol.BatchedOracle(w, n)
    for u in range(n_up):
        got = eng.update(audio[:, u])
        want = ref.update_raw(audio[:, u])
        assert not np.isnan(got).any(), u
        assert np.abs(got.astype(np.float64) - want).max() <= GUARD_RAW, u
        assert eng.chain_carry()[1]
    eng.close()
