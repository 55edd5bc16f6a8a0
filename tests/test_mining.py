"""GPU: the mining session (csrc/mine_device.h, pe_miner) against the per-chunk public API it replaces.

Every comparison is equality: a scan is pe_predict's arithmetic over the frames the offline front end computes, which is what a
float-mode ``Listener`` runs per chunk; a hit's rows are pe_vectorize_clips' launch over the saved ring; the trainer sees the
same float32 rows in the same order.  The expected rings, chunk counts and the policy come from incremental_reference.py; the
hit ids of a session too large for a Listener (66 compaction blocks) come from numpy's comparison over the scores it returned.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import incremental_reference as ref
from mycroft_precise_amd import params as P
from mycroft_precise_amd import synth
from mycroft_precise_amd._lib import HipEngine, HipMiner
from mycroft_precise_amd.mining import Miner
from mycroft_precise_amd.model import ModelParams, save_weights
from mycroft_precise_amd.network_runner import HipRunner, Listener
from mycroft_precise_amd.threshold_decoder import ThresholdDecoder
from mycroft_precise_amd.train import IncrementalTrainer, Trainer

pytestmark = pytest.mark.gpu

THREE_S = 47000


def recording(s, n):
    """load_audio's output for a synthetic wav: k / 32767 in float32"""
    return synth.stream_pcm(s, n).astype(np.float32) / np.float32(32767.0)


def recordings(C):
    return [recording(s, n) for s, n in enumerate([0, 1, C - 1, C, C + 1, 2 * C, 2 * C + 1, THREE_S])]


@functools.lru_cache(maxsize=None)
def weights(seed=7):
    return synth.make_weights(P.pr.n_mfcc, (20,), seed=seed)


@pytest.fixture(scope='module')
def model_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('mining') / 'random20.npz')
    save_weights(path, weights())
    return path


def listener_scores(lis, audios, C):
    """raw outputs of a Listener fed every chunk, cleared per recording (scripts/train_incremental.py:119-124)"""
    out = []
    for audio in audios:
        lis.clear()
        for chunk in ref.chunks(audio, C):
            out.append(np.float32(lis.update_raw(chunk)))
            assert lis._float_mode
    return np.asarray(out, dtype=np.float32)


# ---- scan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,passes', [(512, 1), (1600, 1), (2048, 1), (2048, 3), (24000, 1)])
def test_scan_equals_the_listener_per_chunk(model_file, C, passes):
    audios = recordings(C)
    runner = HipRunner(weights=weights())
    miner = Miner(runner, audios, chunk_size=C)
    assert miner.chunk_offsets.tolist() == ref.chunk_offsets([len(a) for a in audios], C).tolist()
    if passes > 1:      # a window of the batch is 29 x 13 floats: force at least three passes over the session's chunks
        per = -(-miner.n_chunks // passes) - 1
        assert per >= 1 and -(-miner.n_chunks // per) >= 3
        runner.engine.set_clip_pass_bytes(per * P.pr.n_features * P.pr.n_mfcc * 4)
    hits, n_above, scores = miner.scan(return_scores=True)
    want = listener_scores(Listener(model_file, C), audios, C)
    print('C=%d: %d chunks, %d above 0.5' % (C, want.size, n_above))
    assert want.size == miner.n_chunks and want.size >= 3
    assert scores.tobytes() == want.tobytes()
    assert hits.tolist() == np.flatnonzero(want.astype(np.float64) > 0.5).tolist() and n_above == hits.size
    miner.close()


# ---- hits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('decoder', [False, True])
def test_hits_are_the_strict_float64_comparison_in_order(decoder):
    C = 512
    audios = [recording(10 + s, n) for s, n in enumerate([THREE_S, 0, 30000, 700, THREE_S])]
    runner = HipRunner(weights=weights())
    conf_of = lambda s: s.astype(np.float64)
    if decoder:
        dec = ThresholdDecoder(P.pr.threshold_config, P.pr.threshold_center)
        runner.engine.set_decoder(dec)
        conf_of = dec.decode_many
    miner = Miner(runner, audios, chunk_size=C)
    _, _, scores = miner.scan(threshold=2.0, return_scores=True)
    conf = conf_of(scores)
    order = np.argsort(conf, kind='stable')
    pivot = int(order[conf.size // 2])
    thr = float(conf[pivot])                        # the exact float64 value of one prediction near the median
    want = np.flatnonzero(conf > thr)
    hits, n_above, _ = miner.scan(threshold=thr)
    print('%d chunks, %d hits above %r' % (conf.size, want.size, thr))
    assert 0 < want.size < conf.size
    assert pivot not in hits.tolist()
    assert hits.tolist() == want.tolist() and n_above == want.size
    few, n_above, _ = miner.scan(threshold=thr, capacity=3)
    assert few.tolist() == want[:3].tolist() and n_above == want.size
    none, n_above, _ = miner.scan(threshold=thr, capacity=0)
    assert none.size == 0 and n_above == want.size
    first = int(want[1]) + 1                        # a scan from the middle: the same ids, the same scores
    tail, n_tail, tail_scores = miner.scan(first=first, threshold=thr, return_scores=True)
    assert tail.tolist() == want[want >= first].tolist() and n_tail == tail.size
    assert tail_scores.tobytes() == scores[first:].tobytes()
    miner.close()


# ---- hits past one compaction block ------------------------------------------------------------------------------------------
BLOCK = 4096                            # kMineThreads * kMineItems (csrc/mine_device.h): the predictions one compaction block owns
N_BLOCKS_SESSION = 65 * BLOCK + 1       # 66 blocks, one prediction in the last: past the 64 counts mine_scan_counts sums at a time


def mine_blocks(n):
    return -(-n // BLOCK)


@functools.lru_cache(maxsize=None)
def block_session_audios():
    """Recordings with N_BLOCKS_SESSION chunks of ONE sample (a recording of n samples has n - 1 of them), so that the hits of
    a threshold between the scores lie in every block and on both kinds of block boundary whatever the network's last bits:

      * the first window_samples - 1 chunks of every recording see the all-zero window of a cleared Listener and share one
        score, p0; with ``weights()`` the tones of streams 50 .. 59 (mod 97: synth.stream_pcm) score below p0 and those of
        streams 100 .. 139 above it.  Most recordings are of the first kind and between 3600 and 5599 samples long: more than
        half of all chunks score below p0, so the median threshold lies among them, the p0 chunks at the head of every
        recording are hits, and no 4096 consecutive ids are without one;
      * after every third recording a filler of fewer than 4096 chunks makes the next recording start on a multiple of 4096:
        ids 4096 b - 1 (the end of a recording) and 4096 b (p0) are judged independently, where otherwise a run of one hop of
        equal scores straddles the boundary;
      * an empty recording, one below an analysis window and one of a single sample at the head, three chunkless ones in
        the middle.
    The test asserts these properties of the reference hit set; the lengths are drawn with a fixed seed."""
    rng = np.random.default_rng(1)
    specs, total, k = [(50, 0), (51, 700), (52, 1)], 699, 0
    while N_BLOCKS_SESSION - total > 5599:
        n = int(rng.integers(3600, 5600))
        specs.append((100 + k % 40 if k % 9 == 3 else 50 + k % 10 + 97 * (k // 10 % 3), n))
        total += n - 1
        k += 1
        filler = -total % BLOCK
        if k % 3 == 0 and filler and N_BLOCKS_SESSION - total - filler > 5599:
            specs.append((50 + k % 10 + 97 * 3, filler + 1))
            total += filler
        if k == 20:
            specs += [(53, 0), (54, 1), (55, 0)]
    if N_BLOCKS_SESSION - total:
        specs.append((59, N_BLOCKS_SESSION - total + 1))
    audios = [recording(s, n) for s, n in specs]
    for a in audios:
        a.setflags(write=False)
    return tuple(audios)


def quantile_value(conf, q):
    """the exact float64 value of one prediction near the q-quantile"""
    return float(np.sort(conf)[int(q * conf.size)])


@pytest.mark.parametrize('decoder', [False, True])
def test_hits_in_order_across_compaction_blocks(decoder):
    audios = block_session_audios()
    lengths = [len(a) for a in audios]
    assert 0 in lengths and any(0 < n < P.pr.window_samples for n in lengths)
    runner = HipRunner(weights=weights())
    conf_of = lambda s: s.astype(np.float64)
    if decoder:
        dec = ThresholdDecoder(P.pr.threshold_config, P.pr.threshold_center)
        runner.engine.set_decoder(dec)

        def conf_of(s):                 # decode_many is element-wise: every distinct prediction once
            values, inverse = np.unique(s, return_inverse=True)
            return dec.decode_many(values)[inverse]
    miner = Miner(runner, audios, chunk_size=1)
    n = miner.n_chunks
    assert n == int(ref.chunk_offsets(lengths, 1)[-1]) == N_BLOCKS_SESSION
    assert miner.chunk_offsets.tolist() == ref.chunk_offsets(lengths, 1).tolist()
    none, n_above, scores = miner.scan(threshold=2.0, return_scores=True)
    assert none.size == 0 and n_above == 0 and scores.size == n
    conf = conf_of(scores)
    assert conf.dtype == np.float64 and conf.shape == (n,)

    def check(thr, first=0, capacity=None, return_scores=False):
        want = first + np.flatnonzero(conf[first:] > thr)
        hits, n_above, got_scores = miner.scan(first=first, threshold=thr, capacity=capacity, return_scores=return_scores)
        assert n_above == want.size
        assert hits.dtype == np.int32 and np.array_equal(hits, want if capacity is None else want[:capacity])
        if return_scores:
            assert got_scores.tobytes() == scores[first:].tobytes()
        return want

    # thresholds: every chunk, none, and the exact values of predictions, so that `>` is strict in every block at once
    everything = check(float('-inf'))
    assert np.array_equal(everything, np.arange(n))
    assert check(float(conf.max())).size == 0
    for q in (0.25, 0.9):
        thr = quantile_value(conf, q)
        want = check(thr)
        print('%d chunks, %d distinct predictions, q = %.2f: %d hits above %r' % (n, np.unique(scores).size, q, want.size, thr))
        assert 0 < want.size < n
    thr = quantile_value(conf, 0.5)
    want = np.flatnonzero(conf > thr)
    total = want.size
    # what the reference hit set must be like for the scans below to leave the first block, before the device is asked
    hit = np.zeros(n, bool)
    hit[want] = True
    edges = BLOCK * np.arange(1, mine_blocks(n))
    both, one = hit[edges - 1] & hit[edges], hit[edges - 1] ^ hit[edges]
    print('median %r: %d hits in %d blocks; boundaries with hits on both sides %d, on one side %d; %d hits from id %d on'
          % (thr, total, np.unique(want // BLOCK).size, both.sum(), one.sum(), np.count_nonzero(want >= 64 * BLOCK), 64 * BLOCK))
    assert np.unique(want // BLOCK).size >= 65
    assert both.any() and one.any()
    assert want[-1] >= 64 * BLOCK
    assert np.array_equal(check(thr), want)
    # capacity: around the total, and cuts inside block 1 and inside a block behind the first 64
    in_block = lambda b: np.count_nonzero(want // BLOCK == b)
    late = max([b for b in range(64, mine_blocks(n)) if in_block(b) >= 2], default=None)
    assert in_block(1) >= 2 and late is not None
    cut_early = np.count_nonzero(want < BLOCK) + in_block(1) // 2
    cut_late = np.count_nonzero(want < late * BLOCK) + in_block(late) // 2
    assert want[cut_early - 1] // BLOCK == 1 == want[cut_early] // BLOCK and want[cut_late - 1] // BLOCK == late == want[cut_late] // BLOCK
    for capacity in (1, total - 1, total, total + 5, cut_early, cut_late):
        check(thr, capacity=capacity)
    # first: 64 full blocks; 65 with one prediction in the last; ids that are odd against the blocks
    for first, blocks, in_last in ((n - 64 * BLOCK, 64, BLOCK), (n - 64 * BLOCK - 1, 65, 1), (BLOCK + 1 + 123, 64, BLOCK - 123)):
        assert mine_blocks(n - first) == blocks and n - first - (blocks - 1) * BLOCK == in_last
        tail = check(thr, first=first, return_scores=True)
        assert np.array_equal(tail, want[want >= first]) and tail.size > 0
    # the same scan twice: the same bytes
    a, b = miner.scan(threshold=thr, return_scores=True), miner.scan(threshold=thr, return_scores=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()
    miner.close()


def test_one_sample_chunks_agree_with_listener_sized_chunks(model_file):
    """Nothing can replay 266 241 chunks through a Listener.  The prediction of a chunk depends on the samples that have arrived
    alone, so chunk j of a recording at C = 512 -- which a Listener does verify -- is chunk 512 (j + 1) - 1 of it at C = 1."""
    C = 512
    audios = block_session_audios()
    lengths = [len(a) for a in audios]
    runner = HipRunner(weights=weights())
    fine, coarse = Miner(runner, audios, chunk_size=1), Miner(runner, audios, chunk_size=C)
    _, _, fine_scores = fine.scan(threshold=2.0, return_scores=True)
    _, _, coarse_scores = coarse.scan(threshold=2.0, return_scores=True)
    off1, offc = ref.chunk_offsets(lengths, 1), ref.chunk_offsets(lengths, C)
    assert fine.chunk_offsets.tolist() == off1.tolist() and coarse.chunk_offsets.tolist() == offc.tolist()
    want = listener_scores(Listener(model_file, C), audios, C)
    assert want.size == coarse.n_chunks >= 400
    assert coarse_scores.tobytes() == want.tobytes()
    same_samples = np.concatenate([off1[r] + C * (np.arange(offc[r + 1] - offc[r]) + 1) - 1 for r in range(len(audios))])
    assert same_samples.size == coarse.n_chunks and np.all(np.diff(same_samples) > 0) and same_samples[-1] < fine.n_chunks
    assert fine_scores[same_samples].tobytes() == coarse_scores.tobytes()
    # between those: a prediction changes only where a frame has been emitted (window and hop from params, not from the kernel)
    bits = fine_scores.view(np.uint32)
    steps = changes = 0
    for r, n in enumerate(lengths):
        mine = bits[off1[r]:off1[r + 1]]
        emitted = ref.emitted_frames(np.arange(1, mine.size + 1), P.pr.window_samples, P.pr.hop_samples)
        assert emitted.size == max(n - 1, 0)
        no_frame = emitted[1:] == emitted[:-1]
        assert np.array_equal(mine[1:][no_frame], mine[:-1][no_frame]), r
        steps += np.count_nonzero(~no_frame)
        changes += np.count_nonzero(mine[1:] != mine[:-1])
    print('%d chunks at C = 1, %d at C = %d; %d frames emitted, %d changes of the prediction' % (fine.n_chunks, coarse.n_chunks, C, steps, changes))
    assert 0 < changes <= steps
    fine.close(); coarse.close()


# ---- the saved rings ------------------------------------------------------------------------------------------------------
def ring_audios():
    """three recordings shorter than the ring (24000 samples) in a row, so that a ring spans them, behind a long first one whose
    first 11 chunks of 2048 leave zeros at the head of the ring"""
    return [recording(20 + s, n) for s, n in enumerate([30000, 5000, 6500, 7000, 0, 26000])]


@pytest.mark.parametrize('carry', [True, False])
def test_vectorize_equals_vectorize_clips_of_the_saved_rings(carry):
    C, B = 2048, P.pr.buffer_samples
    audios = ring_audios()
    runner = HipRunner(weights=weights())
    miner = Miner(runner, audios, chunk_size=C, carry_audio=carry)
    rings = ref.rings(audios, C, B, carry)
    assert len(rings) == miner.n_chunks
    assert np.count_nonzero(rings[3][:B - 4 * C]) == 0 and np.any(rings[3][B - 4 * C:])           # zeros in front
    off = miner.chunk_offsets
    spanning = int(off[3]) + 1                  # a chunk of the third short recording: its ring holds recordings 1, 2 and 3
    assert len(audios[1]) + len(audios[2]) < B and (not carry or np.any(rings[spanning][:B - 2 * C]))
    ids = np.arange(miner.n_chunks)
    clips = [ref.round_trip(r) for r in rings]
    assert any(np.any(c != r.astype(np.float32)) for c, r in zip(clips, rings))
    want = runner.engine.vectorize_clips(clips, P.pr.max_samples)
    got = miner.vectorize(ids)
    assert got.tobytes() == want.tobytes()
    back = miner.vectorize(ids[::-1].copy())    # any order, and in two passes
    runner.engine.set_clip_pass_bytes(B * 4 * (miner.n_chunks // 2 + 1))
    assert miner.vectorize(ids[::-1].copy()).tobytes() == back.tobytes() == want[::-1].tobytes()
    with pytest.raises(ValueError):
        miner.vectorize([miner.n_chunks])
    miner.close()


def chunkless_audios():
    """300 recordings of 0 .. 50 samples at C = 7: lengths 0, 1 and 7 have no chunk, so the prefix table mine_recording_of
    searches holds long runs of equal entries -- at its head, at its tail and in between"""
    rng = np.random.default_rng(17)
    lengths = [0, 1, 7, 0, 1, 7] + rng.choice([0, 1, 7, 8, 15, 50], 289).tolist() + [7, 0, 0, 1, 0]
    return [recording(200 + s, n) for s, n in enumerate(lengths)]


def longest_chunkless_run(lengths, C):
    best = run = 0
    for n in lengths:
        run = run + 1 if ref.n_chunks(n, C) == 0 else 0
        best = max(best, run)
    return best


RING_CASES = {
    # name: (C, B, recordings): B <= max_samples, the ring the script saves
    'chunk_is_the_ring': (24000, 24000, lambda: [recording(60, 2 * 24000 + 1), recording(61, 3 * 24000 + 5)]),
    'chunk_longer_than_the_ring': (30001, 24000, lambda: [recording(62, 2 * 30001 + 1), recording(63, 3 * 30001 + 5)]),
    'one_sample_chunks': (1, 2000, lambda: [recording(64 + s, n) for s, n in enumerate([300, 0, 1, 2, 150, 400])]),
    'ring_below_a_window': (256, 1000, lambda: ring_audios()),
    'many_chunkless_recordings': (7, 24000, chunkless_audios),
}


@pytest.mark.parametrize('carry', [True, False])
@pytest.mark.parametrize('case', sorted(RING_CASES))
def test_saved_rings_at_other_geometries(model_file, case, carry):
    C, B, make = RING_CASES[case]
    audios = make()
    lengths = [len(a) for a in audios]
    runner = HipRunner(weights=weights())
    miner = Miner(runner, audios, chunk_size=C, carry_audio=carry, buffer_samples=B)
    off = ref.chunk_offsets(lengths, C)
    n = miner.n_chunks
    assert miner.chunk_offsets.tolist() == off.tolist() and 0 < n <= 900
    ids = np.arange(n)
    if case == 'many_chunkless_recordings':         # a shuffled subset, repeats included
        ids = np.random.default_rng(23).integers(0, n, 200)
        assert longest_chunkless_run(lengths, C) >= 5 and longest_chunkless_run(lengths[:6], C) == 6 and longest_chunkless_run(lengths[-5:], C) == 5
        assert len(audios) == 300 and set(lengths) == {0, 1, 7, 8, 15, 50}
        want_where = ref.locate(lengths, C)
        rec, chunk = miner.locate(np.arange(n))
        assert list(zip(rec.tolist(), chunk.tolist())) == want_where
    rings = ref.rings(audios, C, B, carry, only=set(ids.tolist()))
    assert len(rings) == n and all(len(rings[i]) == B for i in ids)
    if case in ('chunk_is_the_ring', 'chunk_longer_than_the_ring'):     # the ring is the tail of one chunk, of any recording
        for r, audio in enumerate(audios):
            for i in range(int(off[r + 1] - off[r])):
                assert np.array_equal(rings[int(off[r]) + i], audio[(i + 1) * C - B:(i + 1) * C].astype(np.float64))
    if case == 'one_sample_chunks':
        g = int(off[4]) + 10                        # 11 samples of recording 4 behind recordings 3 (one chunk) and 0 (299)
        assert lengths[1:3] == [0, 1] and off[1] == off[2] == off[3]
        head = rings[g][:B - 11]
        assert np.array_equal(rings[g][B - 11:], audios[4][:11].astype(np.float64))
        if carry:
            assert head[-1] == audios[3][0] and np.array_equal(head[-300:-1], audios[0][:299].astype(np.float64)) and not np.any(head[:-300])
        else:
            assert not np.any(head)
    clips = [ref.round_trip(rings[i]) for i in ids]
    want = runner.engine.vectorize_clips(clips, P.pr.max_samples)
    got = miner.vectorize(ids)
    assert got.shape == want.shape == (ids.size, P.pr.n_features, P.pr.n_mfcc)
    assert got.tobytes() == want.tobytes()
    if case == 'ring_below_a_window':               # no frame fits into the ring: every row of every hit is padding
        assert B < P.pr.window_samples and any(np.any(c) for c in clips)
        assert want.tobytes() == np.zeros_like(want).tobytes()
        T, F = P.pr.n_features, P.pr.n_mfcc
        rng = np.random.default_rng(5)
        X = rng.normal(0, 1, (7, T, F)).astype(np.float32)
        y = (rng.random(7) < 0.5).astype(np.float32)
        trainer = Trainer(weights(), ModelParams(recurrent_units=20), n_features=T)
        some = np.array([0, n - 1, int(off[3]) + 1, 5, 5])
        for validation in (False, True):
            trainer.set_data(X, y, validation=validation)
            miner.append_to(trainer, some, validation=validation)
            feats, targets = trainer._t.get_data(validation=validation)
            assert feats[:7].tobytes() == X.tobytes() and targets[:7].tobytes() == y.tobytes()
            assert feats[7:].tobytes() == np.zeros((some.size, T, F), np.float32).tobytes() and np.all(targets[7:] == 0.0)
        trainer.close()
    else:
        assert np.any(want)
    if case == 'many_chunkless_recordings' and carry:       # the same table in mine_gather: under a thousand Listener updates
        _, _, scores = miner.scan(threshold=2.0, return_scores=True)
        assert scores.tobytes() == listener_scores(Listener(model_file, C), audios, C).tobytes()
    miner.close()


def add_deltas32(x):
    """the delta columns as pe_score_clips forms them: float32 differences of the padded window, zero in its first row"""
    d = np.zeros_like(x)
    d[:, 1:] = x[:, 1:] - x[:, :-1]
    return np.concatenate([x, d], axis=-1)


@pytest.mark.parametrize('shape', ['stock', 'use_delta', 'general'])
def test_append_puts_the_rows_behind_the_resident_set(shape):
    hpr = P.pr.copy()
    if shape == 'use_delta':
        hpr.__dict__['use_delta'] = True
    if shape == 'general':                          # a non-stock .params shape: the general front end
        hpr.__dict__.update(n_fft=1024, n_filt=40, n_mfcc=20)           # (rows of 32 floats)
    F = hpr.n_mfcc * (2 if hpr.use_delta else 1)
    T, B, C = hpr.n_features, hpr.buffer_samples, 2048
    w = synth.make_weights(F, (20,), seed=3)
    eng = HipEngine(hpr, w)
    audios = ring_audios()
    miner = Miner(SimpleNamespace(engine=eng), audios, chunk_size=C, buffer_samples=B)
    rng = np.random.default_rng(5)
    X = rng.normal(0, 1, (7, T, F)).astype(np.float32)
    y = (rng.random(7) < 0.5).astype(np.float32)
    ids = np.array([0, 5, int(miner.chunk_offsets[3]) + 1, miner.n_chunks - 1, 5])
    rows = miner.vectorize(ids)
    clips = [ref.round_trip(ref.rings(audios, C, B)[i]) for i in ids]
    assert rows.tobytes() == eng.vectorize_clips(clips, hpr.max_samples).tobytes()
    want = rows.astype(np.float32)
    if hpr.use_delta:
        want = add_deltas32(want)
    for validation in (False, True):
        trainer = Trainer(w, ModelParams(recurrent_units=20), n_features=T)
        trainer.set_data(X, y, validation=validation)
        miner.append_to(trainer, ids[:2], validation=validation)
        miner.append_to(trainer, ids[2:], validation=validation)
        assert trainer.n_samples(validation) == 7 + ids.size and trainer.n_samples(not validation) == 0
        feats, targets = trainer._t.get_data(validation=validation)
        assert feats[:7].tobytes() == X.tobytes() and targets[:7].tobytes() == y.tobytes()
        assert feats[7:].tobytes() == want.tobytes()
        assert np.all(targets[7:] == 0.0)
        trainer.close()
    other = Trainer(synth.make_weights(F + 1, (20,), seed=3), ModelParams(recurrent_units=20), n_features=T)
    with pytest.raises(ValueError):
        miner.append_to(other, ids)
    miner.close()


def test_fit_resident_equals_fit_on_the_concatenated_arrays():
    C = 2048
    audios = ring_audios()
    runner = HipRunner(weights=weights())
    miner = Miner(runner, audios, chunk_size=C)
    rng = np.random.default_rng(11)
    T, F = P.pr.n_features, P.pr.n_mfcc
    X = rng.normal(0, 1, (9, T, F)).astype(np.float32)
    y = (rng.random(9) < 0.5).astype(np.float32)
    Xv = rng.normal(0, 1, (4, T, F)).astype(np.float32)
    ids = np.arange(0, miner.n_chunks, 3)
    new = miner.vectorize(ids).astype(np.float32)
    a = Trainer(weights(), ModelParams(recurrent_units=20), seed=9)
    a.set_data(X[:5], y[:5])
    a.append(X[5:], y[5:])                          # the host append, then the device one
    a.set_data(Xv, np.zeros(4, np.float32), validation=True)
    miner.append_to(a, ids)
    ha = a.fit_resident(batch_size=8, epochs=2, shuffle=False)
    b = Trainer(weights(), ModelParams(recurrent_units=20), seed=9)
    hb = b.fit(np.concatenate([X, new]), np.concatenate([y, np.zeros(ids.size, np.float32)]), batch_size=8, epochs=2, shuffle=False,
               validation_data=(Xv, np.zeros(4, np.float32)))
    assert a._t.get_weights().tobytes() == b._t.get_weights().tobytes()
    assert a._t.get_accumulators().tobytes() == b._t.get_accumulators().tobytes()
    assert ha['loss'] == hb['loss'] and sorted(ha) == sorted(hb)
    assert np.any(a._t.get_weights() != Trainer(weights(), ModelParams(recurrent_units=20), seed=9)._t.get_weights())
    miner.close()


# ---- set_weights ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['auto', 'tiling0', 'bf16', 'model1of2', 'projection'])
def test_set_weights_gives_the_bits_of_an_engine_created_with_them(form):
    w1, w2, w3 = weights(1), weights(2), weights(3)
    kw = dict(gru_precision='bf16') if form == 'bf16' else {}
    multi = form == 'model1of2'
    live = HipEngine(P.pr, [w3, w1] if multi else w1, n_streams=3, **kw)
    fresh = HipEngine(P.pr, [w3, w2] if multi else w2, n_streams=3, **kw)
    old = HipEngine(P.pr, [w3, w1] if multi else w1, n_streams=3, **kw)
    if form == 'tiling0':
        for e in (live, fresh, old):
            e.set_gru_tiling(0)
    if form == 'projection':                        # x.W + b stored per frame: rebuilt from the new network, for the frames in the ring too
        for e in (live, fresh, old):
            e.set_input_projection(True)
    pcm = synth.batch_pcm(3, 40, 1024)
    for u in range(30):                             # streams in progress, on the old network
        a, b = live.update(pcm[u]), fresh.update(pcm[u])
        old.update(pcm[u])
    assert a.tobytes() != b.tobytes()
    window = live.get_vectors()
    live.set_weights(w2, model=1 if multi else 0)
    assert live.get_vectors().tobytes() == window.tobytes() == fresh.get_vectors().tobytes()
    for u in range(30, 40):
        assert live.update(pcm[u]).tobytes() == fresh.update(pcm[u]).tobytes()
    x = np.random.default_rng(0).normal(0, 1, (37, P.pr.n_features, P.pr.n_mfcc)).astype(np.float32)
    assert live.predict(x).tobytes() == fresh.predict(x).tobytes()
    audios = recordings(2048)
    model = 1 if multi else 0
    ma, mb = HipMiner(live, audios, 2048, P.pr.buffer_samples), HipMiner(fresh, audios, 2048, P.pr.buffer_samples)
    sa, sb = ma.scan(return_scores=True, model=model), mb.scan(return_scores=True, model=model)
    assert sa[2].tobytes() == sb[2].tobytes() and sa[0].tolist() == sb[0].tolist() and sa[2].size == ma.n_chunks > 0
    ma.close(); mb.close()
    # a network of other widths is refused and the engine keeps serving what it has
    with pytest.raises(ValueError):
        live.set_weights(synth.make_weights(P.pr.n_mfcc, (16,), seed=1), model=model)
    with pytest.raises(ValueError):
        live.set_weights(w1, model=5)
    assert live.predict(x).tobytes() == fresh.predict(x).tobytes()
    assert live.predict(x).tobytes() != old.predict(x).tobytes()


def test_scan_of_a_k_model_engine_is_each_model_alone():
    """pe_predict_device of a K-model engine writes [K][k] per pass; the scan keeps block `model` of it.  The reference is an
    engine that holds that model alone (the bit equality tests/test_multi_model.py establishes for predict)."""
    C, B = 2048, P.pr.buffer_samples
    T, F = P.pr.n_features, P.pr.n_mfcc
    networks = [weights(1), weights(2), weights(3)]
    audios = recordings(C) + [recording(9, 40000)]
    alone = []
    for w in networks:
        miner = HipMiner(HipEngine(P.pr, w), audios, C, B)
        _, _, scores = miner.scan(threshold=2.0, return_scores=True)
        conf = scores.astype(np.float64)
        thr = quantile_value(conf, 0.5)
        hits, n_above, _ = miner.scan(threshold=thr)
        assert hits.tolist() == np.flatnonzero(conf > thr).tolist() and 0 < hits.size == n_above < conf.size
        alone.append((scores, thr, hits))
        miner.close()
    n = alone[0][0].size
    assert n >= 40
    for a in range(3):
        for b in range(a):
            assert np.any(alone[a][0] != alone[b][0])
    engine = HipEngine(P.pr, networks)
    miner = HipMiner(engine, audios, C, B)
    assert miner.n_chunks == n
    for per in (None, 16):
        if per:                                     # at least three passes, the last shorter than the others: k changes
            assert n > 2 * per and n % per
            engine.set_clip_pass_bytes(per * T * F * 4)
        for model, (scores, thr, hits) in enumerate(alone):
            got_hits, n_above, got_scores = miner.scan(threshold=thr, return_scores=True, model=model)
            assert got_scores.tobytes() == scores.tobytes(), (per, model)
            assert got_hits.tolist() == hits.tolist() and n_above == hits.size, (per, model)
    miner.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_incremental_trainer_equals_the_per_chunk_loop(model_file):
    C, B, delay, epochs, batch = 2048, P.pr.buffer_samples, 3, 1, 16
    T, F = P.pr.n_features, P.pr.n_mfcc
    audios = [recording(40 + s, n) for s, n in enumerate([30000, 21000, 47000, 0, 33000, 26000, 40000])]
    # the first recording is a test recording: the untrained network judges it, its hits push the count past delay_samples, and
    # the first retrain comes at the first chunk of the next recording
    flags = [True, False, False, False, True, False, False]
    rng = np.random.default_rng(21)
    X = rng.normal(0, 1, (24, T, F)).astype(np.float32)
    y = (rng.random(24) < 0.5).astype(np.float32)
    Xv = rng.normal(0, 1, (6, T, F)).astype(np.float32)
    yv = (rng.random(6) < 0.5).astype(np.float32)

    runner = HipRunner(weights=weights())
    probe = Miner(runner, audios, chunk_size=C)
    _, _, scores = probe.scan(return_scores=True)
    probe.close()
    threshold = float(np.sort(scores.astype(np.float64))[int(0.1 * scores.size)])       # most chunks fire until training bites

    trainer = Trainer(weights(), ModelParams(recurrent_units=20), seed=5)
    trainer.set_data(X, y)
    trainer.set_data(Xv, yv, validation=True)
    inc = IncrementalTrainer(trainer, runner, delay_samples=delay, epochs=epochs, batch_size=batch, threshold=threshold, chunk_size=C,
                             capacity=2, shuffle=False)
    got_hits, got_retrains = inc.run(audios, test_flags=flags)

    # the loop a user writes today: Listener.update per chunk, vectorize_clips of host-built rings, fit with a new upload, a new runner
    lis = Listener(model_file, C)
    other = Trainer(weights(), ModelParams(recurrent_units=20), seed=5)

    def retrain(saved):
        rows = lambda test: [r for r, t in saved if t == test]
        new = lis._engine.vectorize_clips(rows(False), P.pr.max_samples).astype(np.float32).reshape(-1, T, F)
        val = lis._engine.vectorize_clips(rows(True), P.pr.max_samples).astype(np.float32).reshape(-1, T, F)
        other.fit(np.concatenate([X, new]), np.concatenate([y, np.zeros(len(new), np.float32)]), batch_size=batch, epochs=epochs,
                  shuffle=False, validation_data=(np.concatenate([Xv, val]), np.concatenate([yv, np.zeros(len(val), np.float32)])))
        lis.runner = HipRunner(weights=other.weights)

    hits, retrains, saved, count = ref.policy_loop(audios, flags, C, B, delay, epochs, threshold, lambda r: lis.clear(),
                                                   lambda r, i, chunk: lis.update_raw(chunk), retrain)
    print('%d chunks, %d hits (%d test), %d retrains' % (scores.size, len(hits), sum(t for _, _, t in hits), len(retrains)))
    assert len(retrains) >= 2 and retrains[0] == (1, 0) and any(t for _, _, t in hits) and any(not t for _, _, t in hits)
    assert got_hits == hits and got_retrains == retrains and inc.samples_since_train == count
    assert trainer._t.get_weights().tobytes() == other._t.get_weights().tobytes()
    assert trainer.n_samples() == 24 + sum(1 for _, _, t in hits if not t) and trainer.n_samples(True) == 6 + sum(1 for _, _, t in hits if t)


def test_the_library_checks_its_arguments_itself():
    """the checks the header promises, through the C ABI directly (the Python classes refuse most of these earlier)"""
    import ctypes as C
    eng = HipEngine(P.pr, weights())
    miner = HipMiner(eng, recordings(2048), 2048, P.pr.buffer_samples)
    lib, h = miner._lib, miner._h
    n = miner.n_chunks
    n_hits, n_above = C.c_int32(-1), C.c_int64(-1)
    hits = np.zeros(4, np.int32)
    scan = lambda first, thr: lib.pe_miner_scan(h, 0, first, thr, None, hits.ctypes.data, 4, C.byref(n_hits), C.byref(n_above))
    INVALID = 1
    assert scan(0, float('nan')) == INVALID and b'NaN' in lib.pe_last_error(eng._h)
    assert scan(n + 1, 0.5) == INVALID and scan(-1, 0.5) == INVALID
    assert lib.pe_miner_scan(h, 1, 0, 0.5, None, hits.ctypes.data, 4, C.byref(n_hits), C.byref(n_above)) == INVALID      # model
    assert lib.pe_miner_scan(h, 0, 0, 0.5, None, None, 4, C.byref(n_hits), C.byref(n_above)) == INVALID                   # capacity without room
    assert scan(n, 0.5) == 0 and n_hits.value == 0 and n_above.value == 0                                                # nothing left: fine
    out = np.full((2, P.pr.n_features, P.pr.n_mfcc), 7.0)
    for bad in ([0, n], [-1, 0]):
        ids = np.array(bad, np.int32)
        assert lib.pe_miner_vectorize(h, ids.ctypes.data, 2, out.ctypes.data) == INVALID
        assert b'outside' in lib.pe_last_error(eng._h) and np.all(out == 7.0)
    trainer = Trainer(weights(), ModelParams(recurrent_units=20))
    ids = np.array([0, n], np.int32)
    assert lib.pe_miner_append(h, trainer._t._h, 1, ids.ctypes.data, 2, 0.0) == INVALID and trainer.n_samples() == 0
    ids = np.array([0, 1], np.int32)
    assert lib.pe_miner_append(h, trainer._t._h, 0, ids.ctypes.data, 2, 0.0) == INVALID            # source: host data is no resident set
    assert lib.pe_miner_append(h, trainer._t._h, 1, ids.ctypes.data, 2, 1.5) == INVALID            # target
    assert lib.pe_miner_append(h, None, 1, ids.ctypes.data, 2, 0.0) == INVALID
    assert trainer.n_samples() == 0
    m2 = C.c_void_p()
    off = np.array([0, 10, 5], np.int64)
    audio = np.zeros(10, np.float32)
    create = lambda offsets, chunk, buf: lib.pe_miner_create(eng._h, audio.ctypes.data, 1, offsets.ctypes.data, offsets.size - 1, chunk, buf, 1, C.byref(m2))
    assert create(off, 4, 8) == INVALID and not m2.value                                             # decreasing offsets
    assert create(np.array([0, 10], np.int64), 0, 8) == INVALID and create(np.array([0, 10], np.int64), 4, 0) == INVALID
    assert create(np.array([1, 10], np.int64), 4, 8) == INVALID
    # an engine that is closed takes its sessions with it; the session then refuses by name
    eng.close()
    with pytest.raises(ValueError):
        miner.scan()
    with pytest.raises(ValueError):
        Miner(HipRunner(weights=weights()), recordings(2048), buffer_samples=P.pr.max_samples + 1)


# ---- the script itself: tests/golden/train_incremental.npz (tools/make_script_fixtures.py) ------------------------------------
def test_miner_and_trainer_equal_the_scripts_own_run(stock_weights):
    """TrainIncrementalScript.train_on_audio's own run over four recordings: the scan gives its hits, the hits' rows are
    pe_vectorize_clips of the int16 clips save_audio wrote (the session hands a saved ring out as rows only), and
    IncrementalTrainer, with a recorder in place of the fit, retrains where the script called retrain()."""
    from conftest import golden
    from test_gpu_parity import TOL_DECODE, TOL_RAW
    g = golden('train_incremental.npz')
    audios = ref.fixture_recordings(g)
    C, B, delay, epochs = (int(g[n]) for n in ('chunk_size', 'buffer_samples', 'delay_samples', 'epochs'))
    threshold = float(g['threshold'])
    flags = (g['flag_draws'] > 0.8).tolist()
    hits = [tuple(h) for h in g['hits'].tolist()]
    ids = [int(g['chunk_starts'][r] + i) for r, i, _ in hits]
    assert np.abs(g['conf'] - threshold).min() > TOL_DECODE and len(hits) >= 6 and B == P.pr.buffer_samples

    runner = HipRunner(weights=stock_weights)
    runner.engine.set_decoder(ThresholdDecoder(P.pr.threshold_config, P.pr.threshold_center))
    miner = Miner(runner, audios, chunk_size=C)
    assert miner.chunk_offsets.tolist() == g['chunk_starts'].tolist()
    got, n_above, scores = miner.scan(threshold=threshold, return_scores=True)
    worst = float(np.abs(scores.astype(np.float64) - g['raw'].astype(np.float64)).max())
    print('%d chunks, worst |score - the script\'s raw output| %.3g, %d hits' % (scores.size, worst, got.size))
    assert worst <= TOL_RAW
    assert got.tolist() == ids and n_above == len(ids)
    rec, chunk = miner.locate(got)
    assert list(zip(rec.tolist(), chunk.tolist())) == [(r, i) for r, i, _ in hits]
    clips = [pcm.astype(np.float32) / np.float32(32767.0) for pcm in g['saved']]             # load_audio of what save_audio wrote
    assert miner.vectorize(got).tobytes() == runner.engine.vectorize_clips(clips, P.pr.max_samples).tobytes()
    miner.close()

    T, F = P.pr.n_features, P.pr.n_mfcc
    trainer = Trainer(stock_weights, ModelParams(recurrent_units=20), seed=5)
    trainer.set_data(np.zeros((4, T, F), np.float32), np.zeros(4, np.float32))
    record = []
    trainer.fit_resident = lambda *args, **kw: record.append(trainer.n_samples() - 4 + trainer.n_samples(True))
    inc = IncrementalTrainer(trainer, runner, delay_samples=delay, epochs=epochs, threshold=threshold, chunk_size=C)
    got_hits, got_retrains = inc.run(audios, test_flags=flags)
    assert [(r, i, int(t)) for r, i, t in got_hits] == hits
    assert [(r, i, n) for (r, i), n in zip(got_retrains, record)] == [tuple(x) for x in g['retrains'].tolist()]
    assert inc.samples_since_train == int(g['samples_since_train'])
    assert trainer.n_samples() == 4 + sum(1 for h in hits if not h[2]) and trainer.n_samples(True) == sum(1 for h in hits if h[2])
    feats, targets = trainer._t.get_data(first=4)
    want = runner.engine.vectorize_clips([c for c, h in zip(clips, hits) if not h[2]], P.pr.max_samples).astype(np.float32)
    assert feats.tobytes() == want.reshape(feats.shape).tobytes() and not targets.any()
