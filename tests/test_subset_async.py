"""
-m gpu: the host-fed pipeline for streams that advance on their own (pe_update_subset_async, pe_decode_subset).

70 streams (four full tiles and one of six) of tone_noise, zeros, square and quiet audio; every stream reads its own audio
front to back, however the rounds group the streams.  The pipeline must give the bits of the synchronous calls it is made of:
pe_update_subset for the raw outputs, pe_decode for the confidences, and one host TriggerDetector per (model, stream) that
sees only the rounds its stream took part in for the activations.
"""
import functools
import warnings

import numpy as np
import pytest

from mycroft_precise_amd import synth
from mycroft_precise_amd import params as P
from mycroft_precise_amd._lib import HipEngine, PE_ERR_INVALID
from mycroft_precise_amd.runner import TriggerDetector
from mycroft_precise_amd.threshold_decoder import ThresholdDecoder

N = 70
CHUNK = 1024
KINDS = ('tone_noise', 'zeros', 'tone_noise', 'square', 'tone_noise', 'quiet', 'tone_noise')
TOTAL = 64 * CHUNK


@functools.lru_cache(maxsize=None)
def _audio():
    """[N][TOTAL] int16, read-only: stream s's audio, consumed front to back by whoever feeds stream s"""
    a = np.stack([synth.stream_pcm(s, TOTAL, KINDS[s % len(KINDS)]) for s in range(N)])
    a.setflags(write=False)
    return a


class Feeder:
    """hands every stream the next samples of its own audio"""

    def __init__(self):
        self.at = np.zeros(N, dtype=np.int64)

    def take(self, ids, chunk=CHUNK):
        a = _audio()
        rows = np.stack([a[s, self.at[s]:self.at[s] + chunk] for s in ids])
        assert rows.shape == (len(ids), chunk), 'the test ran out of audio'
        self.at[np.asarray(ids)] += chunk
        return rows


def _subsets(rng, rounds, fixed=()):
    """`rounds` random subsets of sizes 1..N in random order; fixed: {round: size}"""
    out = []
    for r in range(rounds):
        k = dict(fixed).get(r, int(rng.integers(1, N + 1)))
        out.append(rng.permutation(N)[:k].astype(np.int32))
    return out


def _engine(kind, stock):
    kw = {}
    weights = stock
    if kind == 'bf16':
        kw['gru_precision'] = 'bf16'
    elif kind == 'three_models':
        weights = [stock, synth.make_weights(seed=501), synth.make_weights(seed=502)]
    elif kind == 'wide64':
        weights = synth.make_weights(n_in=13, units=(64,), seed=500)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        e = HipEngine(P.pr, weights, n_streams=N, **kw)
    if kind == 'unfused':
        e.set_fused(False)
    if kind == 'chains':
        e.set_chain_carry(2)
    return e


class Pinned:
    """a rotation of four pinned buffers: one is reused only after the update that used it has been delivered"""

    def __init__(self, eng, n, dtype):
        self.bufs = [eng.host_array((n,), dtype) for _ in range(4)]
        self.i = 0

    def next(self, n):
        self.i += 1
        return self.bufs[self.i % 4][:n]


class InFlight:
    """results of enqueued updates, compared once they have been delivered: by the third later enqueue, or by wait()"""

    def __init__(self):
        self.items = []
        self.checked = 0

    def add(self, got, want, what):
        self.items.append((got, want, what))
        self.check(len(self.items) - 3)

    def check(self, upto=None):
        upto = len(self.items) if upto is None else upto
        while self.checked < upto:
            got, want, what = self.items[self.checked]
            for g, w, name in zip(got, want, ('raw', 'conf', 'fired')):
                if w is None:
                    continue
                assert g.dtype == w.dtype, (what, name)
                assert np.array_equal(np.asarray(g).reshape(np.shape(w)), w), (what, name)
            self.items[self.checked] = None                      # (a pinned buffer behind `got` is about to be reused)
            self.checked += 1


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['stock', 'unfused', 'bf16', 'three_models', 'wide64', 'chains'])
def test_raw_outputs_are_those_of_the_synchronous_subset_path(kind, stock_weights):
    a, b = _engine(kind, stock_weights), _engine(kind, stock_weights)
    K = a.n_models
    rng = np.random.default_rng(2024)
    subsets = _subsets(rng, 40, fixed={3: 1, 5: N, 17: 1, 30: N})
    feed = Feeder()
    pcm_pin, out_pin = Pinned(b, N * CHUNK, '<i2'), Pinned(b, K * N, np.float32)
    flight = InFlight()

    def full(r):
        pcm = feed.take(range(N))
        want = a.update(pcm)
        if r % 2:
            p = pcm_pin.next(N * CHUNK).reshape(N, CHUNK)
            p[:] = pcm
            pcm = p
        flight.add((b.update_async(pcm, out_pin.next(K * N) if r % 4 < 2 else None),), (want,), 'full update in round %d' % r)

    for r, ids in enumerate(subsets):
        for i in range({7: 2, 21: 1, 33: 1}.get(r, 0)):   # full updates in between (two in a row: the leftovers stay in the slots)
            full(r + i)
        if r == 13:                                   # a synchronous reader while updates are in flight
            assert np.array_equal(a.get_vectors(), b.get_vectors())
            flight.check()
        if r == 21:                                   # (right behind a full update: its kept leftovers move to the carry first)
            mask = np.zeros(N, np.uint8)
            mask[::3] = 1
            a.clear(mask)
            b.clear(mask)
            flight.check()
        pcm = feed.take(ids)
        want = a.update_subset(ids, pcm)
        if r % 2 == 0:
            p = pcm_pin.next(ids.size * CHUNK).reshape(ids.size, CHUNK)
            p[:] = pcm
            pcm = p
        out = out_pin.next(K * ids.size) if r % 3 == 0 else None
        got = b.update_subset_async(ids, pcm, out)
        if out is not None:
            assert got is out
        flight.add((got,), (want,), 'round %d, %d streams' % (r, ids.size))
        if kind == 'chains':                          # (eager: every eligible update leaves the chains current)
            assert a.chain_carry() == (2, True) and b.chain_carry() == (2, True), r
    b.wait()
    flight.check()
    for x, y in zip(a.stream_state(), b.stream_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.get_vectors(), b.get_vectors())


@pytest.mark.gpu
def test_one_call_per_chunk_length(stock_weights):
    a, b = _engine('stock', stock_weights), _engine('stock', stock_weights)
    rng = np.random.default_rng(5)
    feed = Feeder()
    flight = InFlight()
    for r, chunk in enumerate((CHUNK, CHUNK, 1, 399, 1500, CHUNK, 1, 399, 1500, CHUNK, CHUNK)):
        if r == 6:                                    # a full update leaves its leftovers in the slot; a 1-sample subset call follows
            pcm = feed.take(range(N))
            flight.add((b.update_async(pcm),), (a.update(pcm),), 'full')
        ids = rng.permutation(N)[:int(rng.integers(1, N + 1))].astype(np.int32)
        pcm = feed.take(ids, chunk)
        flight.add((b.update_subset_async(ids, pcm),), (a.update_subset(ids, pcm),), 'chunk of %d in call %d' % (chunk, r))
    b.wait()
    flight.check()
    for x, y in zip(a.stream_state(), b.stream_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.get_vectors(), b.get_vectors())


# ---- subset decode ------------------------------------------------------------------------------------------------

TRIGGERS = {1: [(4096, 0.5, 1)], 3: [(2048, 0.5, 3), (8192, 0.2, 0), (1024, 0.8, 1)]}       # (chunk_size bytes, sensitivity, level)


def _crafted(rng, m, ids, r):
    """raw outputs of model m for the streams `ids` in round r: bursts near 1 between lulls near 0"""
    burst = np.sin((np.asarray(ids) * 0.7 + r + 7 * m) / 5.0) > 0.2
    return np.clip(np.where(burst, 1 - 1e-4 * rng.random(len(ids)), 1e-3 * rng.random(len(ids))), 1e-7, 1 - 1e-7).astype(np.float32)


def _crafted_rounds(K, rounds=60, seed=77):
    rng = np.random.default_rng(seed)
    out = []
    for r, ids in enumerate(_subsets(rng, rounds)):
        out.append((ids, np.stack([_crafted(rng, m, ids, r) for m in range(K)])))
    return out


def run_detectors(K, rounds, conf_of):
    """One host TriggerDetector per (model, stream), fed conf_of(r)[m][i] in the rounds stream ids[i] takes part in.
    -> (fired per round [K][n_active], events: activations, re-arms (a parked counter back at zero), rounds of a stream
    without activation, streams that sat out a round between two of their hot rounds)"""
    dets = [[TriggerDetector(*TRIGGERS[K][m]) for _ in range(N)] for m in range(K)]
    fired, ev = [], dict(activations=0, rearms=0, silent=0)
    hot_rounds = [[] for _ in range(N)]
    took_part = np.zeros((len(rounds), N), bool)
    for r, (ids, _) in enumerate(rounds):
        conf = conf_of(r)
        f = np.zeros((K, len(ids)), bool)
        took_part[r, ids] = True
        for m in range(K):
            for i, s in enumerate(ids):
                d = dets[m][s]
                before = d.activation
                f[m, i] = d.update(float(conf[m][i]))
                ev['activations'] += int(f[m, i])
                ev['silent'] += int(not f[m, i])
                ev['rearms'] += int(before < 0 <= d.activation)
                if m == 0 and float(conf[m][i]) > 1.0 - d.sensitivity:
                    hot_rounds[s].append(r)
        fired.append(f)
    ev['sat_out'] = sum(any(not took_part[h0 + 1:h1, s].all() for h0, h1 in zip(hot_rounds[s], hot_rounds[s][1:]) if h1 > h0 + 1)
                        for s in range(N))
    return fired, ev


def _decode_engine(K, stock):
    weights = [stock, synth.make_weights(seed=501), synth.make_weights(seed=502)][:K]
    e = HipEngine(P.pr, weights if K > 1 else stock, n_streams=N)
    e.set_decoder(ThresholdDecoder(P.pr.threshold_config, P.pr.threshold_center))
    for m, t in enumerate(TRIGGERS[K]):
        e.set_trigger(*t, model=m if K > 1 else None)
    return e


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 3])
def test_subset_decode_moves_only_the_named_streams_triggers(K, stock_weights):
    # every stream in order: pe_decode itself -- confidences, activations, and the trigger state as later rounds show it
    e1, e2 = _decode_engine(K, stock_weights), _decode_engine(K, stock_weights)
    rng = np.random.default_rng(3)
    every = np.arange(N, dtype=np.int32)
    n_fired = 0
    for r in range(40):
        raw = np.stack([_crafted(rng, m, every, r) for m in range(K)]).reshape(e1._lead(N))
        c1, f1 = e1.decode(raw, want_fired=True)
        c2, f2 = e2.decode_subset(every, raw, want_fired=True) if r < 30 else e2.decode(raw, want_fired=True)
        assert c1.shape == c2.shape == e1._lead(N) and f1.dtype == f2.dtype == bool
        assert np.array_equal(c1, c2) and np.array_equal(f1, f2), r
        n_fired += int(f1.sum())
    assert n_fired > 0
    e1.close()
    e2.close()
    # random subsets
    rounds = _crafted_rounds(K)
    e = _decode_engine(K, stock_weights)
    got_conf, got_fired = [], []
    for ids, raw in rounds:
        c, f = e.decode_subset(ids, raw.reshape(e._lead(ids.size)), want_fired=True)
        got_conf.append(c.reshape(K, ids.size))
        got_fired.append(f.reshape(K, ids.size))
    want_fired, ev = run_detectors(K, rounds, lambda r: got_conf[r])
    assert ev['activations'] > 0 and ev['rearms'] > 0 and ev['silent'] > 0 and ev['sat_out'] == N, ev
    for r in range(len(rounds)):
        assert np.array_equal(got_fired[r], want_fired[r]), r
    e.close()


# ---- the pipeline with its decode ----------------------------------------------------------------------------------

# threshold 1 - 0.8 = 0.2 lies inside the oracle's confidences for this audio (5 % .. 95 %: 0.008 .. 0.38, median 0.17):
# its host detectors fire 46 times and stay silent 1494 times over the rounds below (counted again in the test)
SENSITIVITY, LEVEL = 0.8, 1
ROUNDS = 40


def _detect_rounds():
    rng = np.random.default_rng(99)
    return [None if r in (9, 10, 28) else ids for r, ids in enumerate(_subsets(rng, ROUNDS, fixed={2: 1, 6: N}))]


def oracle_trigger_counts(stock):
    """the host TriggerDetectors over the oracle listener's outputs for the audio and rounds of the pipeline test
    -> (activations, updates without one)"""
    from oracle import listener as ol
    rounds = _detect_rounds()
    took = np.zeros(N, dtype=np.int64)
    for ids in rounds:
        took[np.arange(N) if ids is None else ids] += 1
    ref = ol.BatchedOracle(stock, N)
    dec = ThresholdDecoder(P.pr.threshold_config, P.pr.threshold_center)
    a = _audio()
    conf = [dec.decode_many(ref.update_raw(a[:, j * CHUNK:(j + 1) * CHUNK]).astype(np.float32)) for j in range(int(took.max()))]
    dets = [TriggerDetector(2048, SENSITIVITY, LEVEL) for _ in range(N)]
    nth = np.zeros(N, dtype=np.int64)
    fired = silent = 0
    for ids in rounds:
        for s in (range(N) if ids is None else ids):
            f = dets[s].update(float(conf[nth[s]][s]))
            nth[s] += 1
            fired += int(f)
            silent += int(not f)
    return fired, silent


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 3])
def test_pipeline_with_decode_equals_update_then_decode(K, stock_weights):
    from mycroft_precise_amd.network_runner import BatchedListener, MultiModelListener
    fired, silent = oracle_trigger_counts(stock_weights)
    assert fired > 0 and silent > 0, (fired, silent)

    def listener():
        if K == 1:
            return BatchedListener(stock_weights, N)
        return MultiModelListener([stock_weights, synth.make_weights(seed=501), synth.make_weights(seed=502)], N, params=P.pr)
    la, lb = listener(), listener()
    for ls in (la, lb):
        ls.set_trigger(2048, SENSITIVITY, LEVEL)
    feed = Feeder()
    flight = InFlight()
    n_fired = n_rows = 0
    for r, ids in enumerate(_detect_rounds()):
        if r == 15:                                  # a synchronous decode between updates in flight: it moves every trigger
            raw = np.full(la.engine._lead(N), 0.999, np.float32)
            ca, fa = la.engine.decode(raw, want_fired=True)
            cb, fb = lb.engine.decode(raw, want_fired=True)
            assert np.array_equal(ca, cb) and np.array_equal(fa, fb)
            flight.check()
        if r == 25:                                  # ... and new trigger settings: every detector starts again
            for ls in (la, lb):
                ls.set_trigger(4096, SENSITIVITY, 0)
            flight.check()
        if ids is None:
            pcm = feed.take(range(N))
            conf, f = la.update_detect(pcm)
            want = (None, conf, f)
            got = lb.update_detect_async(pcm)
        else:
            pcm = feed.take(ids)
            raw = la.update_raw(pcm, streams=ids)
            conf, f = la.engine.decode_subset(ids, raw, want_fired=True)
            want = (raw, conf, f)
            got = lb.update_detect_async(pcm, streams=ids)
        assert got[2].dtype == bool and got[1].dtype == np.float64 and got[0].dtype == np.float32
        flight.add(got, want, 'round %d' % r)
        n_fired += int(f.sum())
        n_rows += f.size
    lb.wait()
    flight.check()
    assert 0 < n_fired < n_rows
    # the subset form of update_detect is the same two calls
    ids = np.array([69, 0, 33], dtype=np.int32)
    pcm = feed.take(ids)
    conf, f = lb.update_detect(pcm, streams=ids)
    raw = la.update_raw(pcm, streams=ids)
    want = la.engine.decode_subset(ids, raw, want_fired=True)
    assert np.array_equal(conf, want[0]) and np.array_equal(f, want[1]) and conf.shape == la.engine._lead(3)


# ---- refusals -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refused_calls_leave_the_engine_as_it_was(stock_weights):
    e, twin = _engine('stock', stock_weights), _engine('stock', stock_weights)
    rng = np.random.default_rng(8)
    feed = Feeder()

    def good_round():
        ids = rng.permutation(N)[:int(rng.integers(1, N + 1))].astype(np.int32)
        pcm = feed.take(ids)
        got = e.update_subset_async(ids, pcm)
        want = twin.update_subset(ids, pcm)
        return got, want

    def native(ids, n_active, pcm, chunk, out, conf=None, fired=None):
        return e._lib.pe_update_subset_async(e._h, None if ids is None else ids.ctypes.data, n_active, pcm.ctypes.data, chunk,
                                             out.ctypes.data, None if conf is None else conf.ctypes.data,
                                             None if fired is None else fired.ctypes.data)
    pcm = np.ascontiguousarray(_audio()[:, :CHUNK])
    out = np.full(N, -1.0, np.float32)
    conf = np.full(N, -1.0, np.float64)
    fired = np.full(N, 7, np.uint8)
    twice, pair = np.array([1, 1], np.int32), np.array([1, 2], np.int32)
    refusals = [
        lambda: native(np.array([3, 9, 3], np.int32), 3, pcm, CHUNK, out) == PE_ERR_INVALID,             # named twice
        lambda: native(np.array([3, N], np.int32), 2, pcm, CHUNK, out) == PE_ERR_INVALID,                # out of range
        lambda: native(np.array([-1], np.int32), 1, pcm, CHUNK, out) == PE_ERR_INVALID,
        lambda: native(None, N - 1, pcm, CHUNK, out) == PE_ERR_INVALID,                                  # every stream, but not n_streams rows
        lambda: native(None, 0, pcm, CHUNK, out) == PE_ERR_INVALID,
        lambda: native(np.arange(N + 1, dtype=np.int32), N + 1, pcm, CHUNK, out) == PE_ERR_INVALID,
        lambda: native(np.arange(3, dtype=np.int32), 3, pcm, CHUNK, out, conf) == PE_ERR_INVALID,        # no decoder yet
        lambda: native(np.arange(3, dtype=np.int32), 3, pcm, CHUNK, out, None, fired) == PE_ERR_INVALID,
        lambda: native(np.arange(3, dtype=np.int32), 0, pcm, CHUNK, out, conf, fired) == 0,              # nobody has audio: a no-op
        lambda: e.update_subset_async(np.zeros(0, np.int32), np.zeros((0, CHUNK), '<i2')).size == 0,
        lambda: e._lib.pe_decode_subset(e._h, twice.ctypes.data, 2, out.ctypes.data, conf.ctypes.data, None) == PE_ERR_INVALID,
        lambda: e._lib.pe_decode_subset(e._h, pair.ctypes.data, 2, out.ctypes.data, conf.ctypes.data, None) == PE_ERR_INVALID,  # no decoder
    ]
    in_flight = [good_round() for _ in range(2)]
    for i, refused in enumerate(refusals):
        assert refused(), i
        in_flight.append(good_round())                # (the refusal came between updates in flight)
    with pytest.raises(ValueError, match='pe_set_decoder'):
        e.update_subset_async([1, 2], pcm[:2], conf=np.zeros(2))
    with pytest.raises(EOFError):
        e.update_subset_async([1, 2], np.zeros((2, 0), '<i2'))
    with pytest.raises(ValueError, match='pe_set_decoder'):
        e.decode_subset([1, 2], np.zeros(2, np.float32))
    in_flight.append(good_round())
    e.wait()
    for i, (got, want) in enumerate(in_flight):
        assert np.array_equal(got, want), i
    assert np.all(out == -1.0) and np.all(conf == -1.0) and np.all(fired == 7)          # no refused call and no no-op wrote anything
    for x, y in zip(e.stream_state(), twin.stream_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(e.get_vectors(), twin.get_vectors())
