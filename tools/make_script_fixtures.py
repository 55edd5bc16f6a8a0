#!/usr/bin/env python3
"""
Write tests/golden/{train_generated,train_incremental,train_sampled,simulate}.npz: what the reference's own scripts
(precise/scripts/train_generated.py, train_incremental.py, train_sampled.py with train.py, simulate.py) compute for small seeded
inputs.

    python tools/make_script_fixtures.py --reference /path/to/mycroft-precise [--only generated,incremental,sampled,simulate]

The script modules import packages they never use on the driven paths (prettyparse, pyache, fitipy, keras, speechpy) and ``wavio``:
the first group is replaced by stub modules, ``wavio`` by the in-memory stand-in of tools/reference_stubs.py, ``sonopy`` by
oracle/sonopy_restated.py where the real package is absent (as oracle/gen_golden.py does).  Each script object is made with
``Class.__new__`` -- its ``__init__`` parses arguments, loads a Keras model and globs folders -- and given the attributes its
methods read.  The seams, all of them names the scripts look up themselves:

  * the script module's own ``random`` is a counter over the committed list of draws; simulate.py's own ``glob`` returns the
    in-memory names, train.py's / train_sampled.py's own ``Fitipy`` is an in-memory file;
  * ``script.listener`` is the reference's ``Listener`` inside a recorder that notes what every call was handed and returned;
    where a network runs it is ``oracle.keras_gru.make_runner_cls(stock weights)`` through the ``runner_cls`` seam, as in
    oracle/gen_golden.py (simulate: the same class, which answers an empty batch of windows with an empty [0, 1] array);
  * ``script.retrain`` is a recorder (no Keras here), ``simulate.Metric`` a subclass that remembers its instances.

Everything between those seams is the reference's code, unmodified.  Nothing of it is copied: the files hold arrays and
provenance strings.  The set order of Python strings enters train_sampled.py's ``islice`` over a set; the tool runs itself with
PYTHONHASHSEED=0 so that two runs write the same arrays.

Audio is int16 and piecewise periodic (every piece one waveform repeated), which deflate packs well; see each ``drive_*``
docstring for what a file holds.
"""
import argparse
import contextlib
import io
import os
import subprocess
import sys
import warnings
from itertools import cycle
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, 'tests', 'golden')
sys.dont_write_bytecode = True              # never write __pycache__ into the reference
sys.path.insert(0, REPO)

from reference_stubs import install_stubs, install_wavio          # noqa: E402

TOL_RAW, TOL_DECODE, GUARD_RAW = 1e-4, 2e-3, 2e-5                  # tests/test_gpu_parity.py
KINDS = ('generated', 'incremental', 'sampled', 'simulate')


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def periodic_pcm(rng, n, amplitude=(800, 8000), piece=(1200, 4000)):
    """int16 [n]: pieces of ``piece`` samples, each one period (40 .. 400 samples) of three harmonics repeated"""
    out = np.zeros(n, dtype=np.int16)
    at = 0
    while at < n:
        length = int(rng.integers(*piece))
        period = int(rng.integers(40, 400))
        t = np.arange(period) / period
        wave = sum(rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * (k * t + rng.random())) for k in (1, int(rng.integers(2, 9)), int(rng.integers(9, 40))))
        wave = np.round(rng.uniform(*amplitude) * wave / np.abs(wave).max()).astype(np.int16)
        take = min(length, n - at)
        out[at:at + take] = np.tile(wave, -(-take // period))[:take]
        at += take
    return out


def offsets(arrays):
    return np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)


class Draws:
    """``random()`` over a list, counting"""

    def __init__(self, values):
        self.values, self.n = list(values), 0

    def random(self):
        self.n += 1
        return self.values[self.n - 1]


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


# ---- train_generated -------------------------------------------------------------------------------------------------------
GEN_CHUNKS = (512, 2048)
LONG_CLIP = 19300           # > 0.8 * buffer_samples = 19200


class VectorRecorder:
    """script.listener of train_generated: the reference's Listener, and a note of every chunk it is handed"""

    def __init__(self, inner, script):
        self.inner, self.script, self.chunks = inner, script, []

    def clear(self):
        self.inner.clear()

    def update_vectors(self, chunk):
        s = self.script
        assert chunk.dtype == np.float64 and np.array_equal(s.audio_buffer[-len(chunk):], chunk)
        vals = s.vals_buffer
        self.chunks.append(dict(audio=np.array(s.audio_buffer[-len(chunk):]), ones=int(np.count_nonzero(vals[-len(chunk):] == 1)),
                                last=int(vals[-1]), max_run=int(s.max_run_length(vals, 1)), vals_len=len(vals), label=-1))
        return self.inner.update_vectors(chunk)


def drive_generated(ref, wavio, out):
    """Per chunk size C (keys end in _C): ``background_pcm`` / ``background_offsets``, ``clip_pcm`` / ``clip_offsets`` (the
    positives first; ``n_positives``), ``draws`` (more than are consumed); per file ``file_draws`` (draws consumed), ``chunk_offsets``; ``taken`` (pool index
    of every clip load_audio was asked for, in order) and ``file_taken`` (how many of them per file); per chunk ``label`` (1, 0,
    -1: nothing yielded), ``ones`` (ones among the chunk's targets), ``last`` (vals_buffer[-1]), ``max_run`` (max_run_length of
    vals_buffer), ``vals_len``; ``audio_ids`` and ``audio``: the merged float64 chunks (the tail of audio_buffer) of every chunk
    of a short file and, of a long one, the first and last two, every fourth, and every chunk whose targets change;
    ``windows`` float64 [n_emitted, 29, 13]: what update_vectors returned for the yielded samples."""
    tg, Listener, pr = ref.train_generated, ref.Listener, ref.pr
    for C in GEN_CHUNKS:
        rng = np.random.default_rng(20261021 + C)
        long_bg = ((LONG_CLIP - 1) // C) * C + LONG_CLIP + 3 * C + 1      # the long clip once in whole chunks, once more, into its silence
        backgrounds = [periodic_pcm(rng, n) for n in (long_bg, C + 1, 2 * C + 1, 8000, 12001)]
        positives = [periodic_pcm(rng, n) for n in (LONG_CLIP, C)]
        negatives = [periodic_pcm(rng, n) for n in (C - 1, 700)]
        clips = positives + negatives
        names = {'bg': ['bg%d.wav' % i for i in range(len(backgrounds))], 'clip': ['clip%d.wav' % i for i in range(len(clips))]}
        wavio.files.clear()
        wavio.files.update(zip(names['bg'] + names['clip'], backgrounds + clips))
        tail = np.random.default_rng(5 + C)
        draws = Draws([0.37, 0.9, 0.1] + tail.random(400).tolist())      # file 0: volume, a positive (the long clip), 0.7 s of silence

        script = tg.TrainGeneratedScript.__new__(tg.TrainGeneratedScript)
        script.args = SimpleNamespace(chunk_size=C, save_prob=0.0)
        script.audio_buffer = np.zeros(pr.buffer_samples, dtype=float)
        script.vals_buffer = np.zeros(pr.buffer_samples, dtype=float)
        recorder = script.listener = VectorRecorder(Listener('', C, runner_cls=lambda x: None), script)
        script.pos_files_it = iter(cycle(names['clip'][:len(positives)]))
        script.neg_files_it = iter(cycle(names['clip'][len(positives):]))
        tg.random = draws.random

        file_draws, file_taken, chunk_counts, taken, windows = [], [], [], [], []
        for fn in names['bg']:
            before, reads, first_chunk = draws.n, len(wavio.reads), len(recorder.chunks)
            for mfccs, target in script.vectors_from_fn(fn):
                assert mfccs.shape == (pr.n_features, pr.n_mfcc) and mfccs.dtype == np.float64
                recorder.chunks[-1]['label'] = int(target)
                windows.append(np.array(mfccs))
            assert wavio.reads[reads] == fn
            new = [names['clip'].index(r) for r in wavio.reads[reads + 1:]]
            taken += new
            file_draws.append(draws.n - before)
            file_taken.append(len(new))
            chunk_counts.append(len(recorder.chunks) - first_chunk)
        chunks = recorder.chunks
        labels = [c['label'] for c in chunks]
        assert set(labels) == {1, 0, -1}, 'C=%d: labels %s' % (C, sorted(set(labels)))
        assert {1, 2} <= set(taken), 'C=%d: the clips of C and C - 1 samples were not both played: %s' % (C, taken)
        assert chunk_counts[1:3] == [1, 2]
        chunk_offsets = np.concatenate([[0], np.cumsum(chunk_counts)]).astype(np.int64)
        audio_ids = []
        for f, n in enumerate(chunk_counts):
            for i in range(n):
                g = int(chunk_offsets[f]) + i
                if n <= 8 or i < 2 or i >= n - 2 or i % 4 == 0 or 0 < chunks[g]['ones'] < C:
                    audio_ids.append(g)
        k = '_%d' % C
        out.update({
            'background_pcm' + k: np.concatenate(backgrounds), 'background_offsets' + k: offsets(backgrounds),
            'clip_pcm' + k: np.concatenate(clips), 'clip_offsets' + k: offsets(clips), 'n_positives' + k: np.int64(len(positives)),
            'draws' + k: np.array(draws.values, dtype=np.float64), 'file_draws' + k: np.array(file_draws, dtype=np.int64),
            'chunk_offsets' + k: chunk_offsets, 'taken' + k: np.array(taken, dtype=np.int64), 'file_taken' + k: np.array(file_taken, dtype=np.int64),
            'audio_ids' + k: np.array(audio_ids, dtype=np.int64), 'audio' + k: np.concatenate([chunks[g]['audio'] for g in audio_ids]),
            'windows' + k: np.array(windows, dtype=np.float64)})
        for name in ('label', 'ones', 'last', 'max_run', 'vals_len'):
            out[name + k] = np.array([c[name] for c in chunks], dtype=np.int64)
        print('generated C=%d: %d chunks, labels %s, %d draws, clips %s, %d audio chunks kept' % (
            C, len(chunks), np.bincount(np.array(labels) + 1).tolist(), draws.n, taken, len(audio_ids)))
    out['buffer_samples'] = np.int64(pr.buffer_samples)
    return 'precise/scripts/train_generated.py (TrainGeneratedScript.vectors_from_fn and what it calls), precise/network_runner.py (Listener), ' \
           'precise/vectorization.py, precise/util.py (load_audio, chunk_audio)'


# ---- train_incremental -----------------------------------------------------------------------------------------------------
INC_CHUNK, INC_DELAY = 2048, 3
INC_LENGTHS = (30000, 26000, 35000, 28000)
INC_FLAG_DRAWS = (0.3, 0.5, 0.9, 0.1)       # random() > 0.8: the third recording is a test recording


class UpdateRecorder:
    """script.listener of train_incremental: the reference's Listener, and a note of every confidence it returned"""

    def __init__(self, inner, runner_cls):
        self.inner, self.runner_cls, self.conf, self.raw, self.starts = inner, runner_cls, [], [], []

    def clear(self):
        self.starts.append(len(self.conf))
        self.inner.clear()

    def update(self, chunk):
        conf = self.inner.update(chunk)
        self.conf.append(float(conf))
        self.raw.append(self.runner_cls.last_raw)
        return conf


def incremental_run(ref, wavio, names, weights, threshold):
    from oracle import keras_gru
    ti, pr = ref.train_incremental, ref.pr

    class Runner(keras_gru.NumpyRunner):
        last_raw = None

        def run(self, inp):
            raw = super().run(inp)
            type(self).last_raw = raw
            return raw
    Runner.weights = weights
    script = ti.TrainIncrementalScript.__new__(ti.TrainIncrementalScript)
    script.args = SimpleNamespace(chunk_size=INC_CHUNK, threshold=threshold, delay_samples=INC_DELAY, epochs=1, folder='data')
    script.audio_buffer = np.zeros(pr.buffer_samples, dtype=float)
    script.samples_since_train = 0
    recorder = script.listener = UpdateRecorder(ref.Listener('synthetic-model-not-on-disk', INC_CHUNK, runner_cls=Runner), Runner)
    retrains = []
    script.retrain = lambda: retrains.append((len(recorder.starts) - 1, len(recorder.conf) - 1 - recorder.starts[-1], len(wavio.written)))
    draws = Draws(INC_FLAG_DRAWS)
    ti.random = draws.random
    del wavio.written[:]
    with quiet():
        for fn in names:
            script.train_on_audio(fn)
    assert draws.n == len(names)
    return recorder, retrains, list(wavio.written), script.samples_since_train


def incremental_policy(conf, starts, flags, threshold):
    """hits, retrains and withheld retrains of a threshold, to choose one (the fixture holds what the script did with it)"""
    count, hits, retrains, withheld = 0, [], 0, 0
    bounds = list(starts) + [len(conf)]
    for r, test in enumerate(flags):
        for i, c in enumerate(conf[bounds[r]:bounds[r + 1]]):
            if c > threshold:
                count += 1
                hits.append((r, i))
            if count >= INC_DELAY:
                if test:
                    withheld += 1
                else:
                    count, retrains = 0, retrains + 1
    return hits, retrains, withheld


def drive_incremental(ref, wavio, out, weights):
    """``pcm`` / ``offsets``: the recordings; ``flag_draws``; ``chunk_size``, ``delay_samples``, ``epochs``, ``threshold``;
    ``chunk_starts`` int64 [n_rec + 1]; per chunk ``conf`` (float64, what Listener.update returned) and ``raw`` (float32, the
    network's output); ``hits`` int64 [n, 3] (recording, chunk, test flag) in the order save_audio was called; ``saved`` int16
    [n, buffer_samples] what it wrote; ``retrains`` int64 [m, 3] (recording, chunk after which retrain() ran, hits saved by
    then); ``samples_since_train`` at the end."""
    pr = ref.pr
    rng = np.random.default_rng(20261022)
    recordings = [periodic_pcm(rng, n) for n in INC_LENGTHS]
    names = ['rec%d.wav' % i for i in range(len(recordings))]
    wavio.files.clear()
    wavio.files.update(zip(names, recordings))
    flags = [d > 0.8 for d in INC_FLAG_DRAWS]
    probe, _, written, _ = incremental_run(ref, wavio, names, weights, float('inf'))
    assert not written
    conf = np.array(probe.conf)
    levels = np.unique(conf)
    chosen = None
    for lo, hi in zip(levels[-2::-1], levels[:0:-1]):           # from the highest gap down: the fewest hits that do
        if hi - lo <= 2 * TOL_DECODE * 1.01:
            continue
        thr = float(round((lo + hi) / 2, 4))
        hits, n_retrains, withheld = incremental_policy(conf, probe.starts, flags, thr)
        early = any(r == 1 and (i + 1) * INC_CHUNK < pr.buffer_samples for r, i in hits)
        if len(hits) >= 6 and early and n_retrains >= 1 and withheld >= 1 and np.abs(conf - thr).min() > TOL_DECODE:
            chosen = thr
            break
    assert chosen is not None, 'no threshold meets the conditions: confidences %s' % levels
    recorder, retrains, written, count = incremental_run(ref, wavio, names, weights, chosen)
    assert recorder.conf == probe.conf and recorder.starts == probe.starts       # nothing retrains: the same confidences
    hits = []
    for name, data in written:
        test = '/test/' in name
        assert name.startswith('data/') and '/not-wake-word/generated/rec' in name and data.shape == (pr.buffer_samples,)
        r, i = os.path.basename(name)[3:-4].split('-')
        hits.append((int(r), int(i), int(test)))
    assert [(r, i) for r, i, _ in hits] == incremental_policy(conf, probe.starts, flags, chosen)[0]
    assert len(hits) >= 6 and retrains and any(t for _, _, t in hits) and np.abs(conf - chosen).min() > TOL_DECODE
    out.update(pcm=np.concatenate(recordings), offsets=offsets(recordings), flag_draws=np.array(INC_FLAG_DRAWS), chunk_size=np.int64(INC_CHUNK),
               delay_samples=np.int64(INC_DELAY), epochs=np.int64(1), threshold=np.float64(chosen), buffer_samples=np.int64(pr.buffer_samples),
               chunk_starts=np.array(recorder.starts + [len(recorder.conf)], dtype=np.int64), conf=conf,
               raw=np.array(recorder.raw, dtype=np.float32), hits=np.array(hits, dtype=np.int64).reshape(-1, 3),
               saved=np.array([d for _, d in written], dtype=np.int16), retrains=np.array(retrains, dtype=np.int64).reshape(-1, 3),
               samples_since_train=np.int64(count))
    print('incremental: %d chunks, threshold %r, hits %s, retrains %s, count %d' % (conf.size, chosen, hits, retrains, count))
    return 'precise/scripts/train_incremental.py (TrainIncrementalScript.train_on_audio), precise/network_runner.py (Listener), ' \
           'precise/threshold_decoder.py, precise/vectorization.py, precise/util.py (load_audio, save_audio, chunk_audio)'


# ---- train_sampled ---------------------------------------------------------------------------------------------------------
SAMPLED_N = 200
SAMPLED_GROUPS = ((5, 50, 120), (10, 11), (30, 199))        # rows with the same input and the same target; the first one fails
SAMPLED_SPLIT = (40, 140)                                   # the same input, different targets: two hashes
SAMPLED_CHUNKS = (10, 1000)                                 # num_sample_chunk of the two cycles


class MemoryFitipy:
    """fitipy's Fitipy over a dict: what train.py and train_sampled.py read and write"""
    store = {}

    def __init__(self, *path):
        self.path = os.path.join(*path)

    def read(self):
        return self

    def write(self):
        return self

    def set(self, value=None):
        if value is None:
            return set(self.store.get(self.path, ()))
        self.store[self.path] = set(value)

    def lines(self, value=None):
        if value is None:
            return list(self.store.get(self.path, ()))
        self.store[self.path] = list(value)


def drive_sampled(ref, out, weights):
    """``inputs`` float64 [n, 29, 13] (multiples of 1/8), ``targets`` float64 [n, 1], ``predictions`` float32 [n, 1] (the
    restated network's, stock weights); ``hash_to_ind`` int64 [n]: the row hash_to_ind holds for row i's hash; per cycle c
    ``num_sample_chunk_c``, ``remaining_c`` (sorted rows, through hash_to_ind, of the script's remaining failed samples),
    ``chosen_c`` (sorted rows of what its islice took), ``n_samples_c`` (len(samples) after the update), ``correct_c`` and
    ``line_c`` (the last line of the metrics file)."""
    from oracle import keras_gru
    ts, train = ref.train_sampled, ref.train
    rng = np.random.default_rng(20261023)
    inputs = np.round(rng.normal(0.0, 3.0, (SAMPLED_N, ref.pr.n_features, ref.pr.n_mfcc)) * 8) / 8
    for group in SAMPLED_GROUPS + (SAMPLED_SPLIT,):
        for row in group[1:]:
            inputs[row] = inputs[group[0]]
    predictions = keras_gru.predict(inputs, weights)
    assert predictions.dtype == np.float32 and predictions.shape == (SAMPLED_N, 1)
    assert np.abs(predictions.astype(np.float64) - 0.5).min() > TOL_RAW
    targets = (predictions > 0.5).astype(np.float64)
    failing = rng.permutation(SAMPLED_N)[:40].tolist()
    failing = (set(failing) - {r for g in SAMPLED_GROUPS[1:] for r in g}) | set(SAMPLED_GROUPS[0]) | {SAMPLED_SPLIT[1]}
    failing -= {SAMPLED_SPLIT[0]}
    for row in failing:
        targets[row] = 1.0 - targets[row]
    train_data = (inputs, targets)

    ts.Fitipy = train.Fitipy = MemoryFitipy
    MemoryFitipy.store.clear()
    script = ts.TrainSampledScript.__new__(ts.TrainSampledScript)
    script.train = train_data
    with quiet():
        script.samples, script.hash_to_ind = ts.TrainSampledScript.load_sample_data('model.samples.json', train_data)
    assert script.samples == set() and len(script.hash_to_ind) == SAMPLED_N - sum(len(g) - 1 for g in SAMPLED_GROUPS)
    script.metrics_fiti = MemoryFitipy('model.logs', 'sampling-metrics.txt')
    hashes = [ref.calc_sample_hash(i, t) for i, t in zip(*train_data)]
    out.update(inputs=inputs, targets=targets, predictions=predictions,
               hash_to_ind=np.array([script.hash_to_ind[h] for h in hashes], dtype=np.int64))
    rows = lambda hs: np.array(sorted(script.hash_to_ind[h] for h in hs), dtype=np.int64)
    for c, chunk in enumerate(SAMPLED_CHUNKS):
        with quiet():
            script.args = SimpleNamespace(num_sample_chunk=10 ** 9)
            remaining = list(script.choose_new_samples(predictions))       # (no side effect: the whole set, to store it)
            script.args = SimpleNamespace(num_sample_chunk=chunk)
            chosen = list(script.choose_new_samples(predictions))
            script.samples.update(chosen)
            script.write_sampling_metrics(predictions)
        assert (len(chosen) == chunk < len(remaining)) if c == 0 else (len(chosen) == len(remaining) < chunk)
        assert set(chosen) <= set(remaining)
        line = script.metrics_fiti.read().lines()[-1]
        out.update({'num_sample_chunk_%d' % c: np.int64(chunk), 'remaining_%d' % c: rows(remaining), 'chosen_%d' % c: rows(chosen),
                    'n_samples_%d' % c: np.int64(len(script.samples)), 'correct_%d' % c: np.float64(line.split('\t')[1]), 'line_%d' % c: np.array(line)})
        print('sampled cycle %d: %d remaining, %d chosen, line %r' % (c, len(remaining), len(chosen), line))
    assert len(script.metrics_fiti.read().lines()) == 2
    return 'precise/scripts/train.py (TrainScript.load_sample_data), precise/scripts/train_sampled.py (choose_new_samples, ' \
           'write_sampling_metrics), precise/util.py (calc_sample_hash)'


# ---- simulate --------------------------------------------------------------------------------------------------------------
SIM_CHUNKS = (1024, 2048, 4096)
SIM_THRESHOLDS = (0.27, 0.265, 0.275, 0.26, 0.28)     # the first that no prediction comes near; not 0.5: `p > t` and `p > 1 - t` differ
# frames f need 1600 + 800 (f - 1) samples, predictions are len(range(29, f, chunk_size // 800)).  29 frames: none; 30: one;
# 92, 93, 94 frames: 63, 64, 65 predictions at chunk_size 1024; 155, 156, 158: 63, 64, 65 at 2048; 340, 345, 350: at 4096
SIM_FRAMES = (29, 30, 92, 93, 94, 155, 156, 158, 340, 345, 350)


def drive_simulate(ref, wavio, out, weights):
    """``pcm`` / ``offsets``: the recordings; ``threshold``; per chunk size C ``predictions_C`` float32 (all recordings'
    concatenated) with ``window_offsets_C``; ``seconds_C``, ``activated_chunks_C``, ``activations_C``, ``activation_sum_C`` per
    recording; ``total_C`` (the same four of the total); ``file_strings_C`` and ``total_string_C``: what run() printed;
    ``string_safe_C`` / ``total_string_safe_C``: the 'Average Activation' figure stays at its two decimals when every
    prediction moves by GUARD_RAW (tests/test_gpu_parity.py: what the device is held to against the oracle)."""
    from oracle import keras_gru
    sim, pr = ref.simulate, ref.pr
    rng = np.random.default_rng(20261024)
    recordings = [periodic_pcm(rng, 1600 + 800 * (f - 1), piece=(800, 3000)) for f in SIM_FRAMES]
    names = ['rec%02d.wav' % i for i in range(len(recordings))]
    wavio.files.clear()
    wavio.files.update(zip(names, recordings))

    class Runner(keras_gru.NumpyRunner):
        def predict(self, inputs):
            if np.asarray(inputs).size == 0:            # a recording without a window: an empty batch
                return np.zeros((0, 1), dtype=np.float32)
            return super().predict(inputs)
    Runner.weights = weights
    created = []

    class Metric(sim.Metric):
        def __init__(self, *args, **kw):
            super().__init__(*args, **kw)
            created.append(self)
    sim.Metric = Metric
    sim.glob = lambda pattern: list(names)

    def run(chunk_size, threshold):
        script = sim.SimulateScript.__new__(sim.SimulateScript)
        script.args = SimpleNamespace(chunk_size=chunk_size, threshold=threshold, folder='noise')
        script.runner = Runner('synthetic-model-not-on-disk')
        predictions = []
        evaluate = script.evaluate
        script.evaluate = lambda audio: predictions.append(evaluate(audio)) or predictions[-1]
        del created[:]
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            script.run()
        return predictions, list(created), printed.getvalue()

    probe = np.concatenate([p.reshape(-1) for C in SIM_CHUNKS for p in run(C, 0.5)[0]]).astype(np.float64)
    levels = np.unique(probe)
    # a threshold t serves `p > t` (activated chunks) and, in the detector, `p > 1 - t` (activations): clear of both
    threshold = None
    for t in SIM_THRESHOLDS:
        if np.abs(probe - t).min() > TOL_RAW and np.abs(probe - (1.0 - t)).min() > TOL_RAW:
            threshold = float(t)
            break
    assert threshold is not None, levels
    out.update(pcm=np.concatenate(recordings), offsets=offsets(recordings), threshold=np.float64(threshold))
    for C in SIM_CHUNKS:
        predictions, metrics, printed = run(C, threshold)
        total, files = metrics[0], metrics[1:]
        assert len(files) == len(recordings) and total.chunk_size == C
        flat = np.concatenate([p.reshape(-1) for p in predictions])
        assert flat.dtype == np.float32 and np.abs(flat.astype(np.float64) - threshold).min() > TOL_RAW
        file_strings = [m.info_string(n) for m, n in zip(files, names)]
        total_string = total.info_string('Total')
        assert all('\n\n' + s + '\n' in printed for s in file_strings) and printed.endswith('\n\n\n' + total_string + '\n')
        counts = [len(p) for p in predictions]
        hot = [int((p.reshape(-1).astype(np.float64) > 1.0 - threshold).sum()) for p in predictions]
        assert any(h > a >= 1 for h, a in zip(hot, (int(m.activations) for m in files))), 'no run of activated chunks is cut by the re-arm'
        assert sum(int(m.activated_chunks) for m in files) > 0 and max(int(m.activations) for m in files) >= 2

        def safe(m, n_windows):
            figure = 100.0 * m.activation_sum / m.chunks
            slack = 100.0 * n_windows * GUARD_RAW / m.chunks
            cents = figure * 100.0
            return bool(abs(cents - np.floor(cents) - 0.5) > slack * 100.0)
        string_safe = [safe(m, n) for m, n in zip(files, counts)]
        k = '_%d' % C
        out.update({
            'predictions' + k: flat, 'window_offsets' + k: np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
            'seconds' + k: np.array([m.seconds for m in files], dtype=np.float64),
            'activated_chunks' + k: np.array([m.activated_chunks for m in files], dtype=np.int64),
            'activations' + k: np.array([m.activations for m in files], dtype=np.int64),
            'activation_sum' + k: np.array([m.activation_sum for m in files], dtype=np.float64),
            'total' + k: np.array([total.seconds, total.activated_chunks, total.activations, total.activation_sum], dtype=np.float64),
            'file_strings' + k: np.array(file_strings), 'total_string' + k: np.array(total_string),
            'string_safe' + k: np.array(string_safe), 'total_string_safe' + k: np.array(safe(total, sum(counts)))})
        print('simulate C=%d: windows %s, activated %s, activations %s, safe strings %d / %d, total safe %s' % (
            C, counts, [int(m.activated_chunks) for m in files], [int(m.activations) for m in files], sum(string_safe), len(string_safe),
            safe(total, sum(counts))))
        if C == 1024:
            assert counts[:5] == [0, 1, 63, 64, 65]
        if C == 2048:
            assert counts[5:8] == [63, 64, 65]
        if C == 4096:
            assert counts[8:] == [63, 64, 65]
    return 'precise/scripts/simulate.py (SimulateScript.run, SimulateScript.evaluate, Metric), runner/precise_runner/runner.py ' \
           '(TriggerDetector), precise/vectorization.py, precise/util.py (load_audio)'


# ---- main ------------------------------------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', required=True, help='a checkout of the reference implementation')
    ap.add_argument('--out', default=OUT, help='the folder the four files go to')
    ap.add_argument('--only', default=','.join(KINDS))
    args = ap.parse_args()
    if os.environ.get('PYTHONHASHSEED') != '0':
        sys.exit(subprocess.run([sys.executable] + sys.argv, env=dict(os.environ, PYTHONHASHSEED='0')).returncode)
    warnings.simplefilter('ignore', DeprecationWarning)        # tostring / fromstring in the reference's util.py

    from oracle import keras_gru, sonopy_restated
    from mycroft_precise_amd import synth
    try:
        import sonopy
        sonopy_note = 'real sonopy %s' % getattr(sonopy, '__version__', '?')
    except ImportError:
        sys.modules['sonopy'] = sonopy_restated
        sonopy_note = 'restated (oracle/sonopy_restated.py), real package not importable'
    stubbed = install_stubs(('prettyparse', 'pyache', 'fitipy', 'keras', 'keras.callbacks', 'keras.models', 'speechpy'))
    reference = os.path.abspath(args.reference)
    sys.path.insert(0, reference)
    sys.path.insert(0, os.path.join(reference, 'runner'))
    from precise.params import pr
    wavio = install_wavio(pr.sample_rate)
    from precise.network_runner import Listener
    from precise.scripts import simulate, train, train_generated, train_incremental, train_sampled
    from precise.util import calc_sample_hash
    ref = SimpleNamespace(pr=pr, Listener=Listener, simulate=simulate, train=train, train_generated=train_generated,
                          train_incremental=train_incremental, train_sampled=train_sampled, calc_sample_hash=calc_sample_hash)
    weights = synth.make_weights()
    stock = np.load(os.path.join(OUT, 'weights_stock_seed42.npz'))
    assert all(np.array_equal(a, stock[n]) for a, n in zip(weights['gru'][0], ('kernel', 'recurrent_kernel', 'bias')))
    assert np.array_equal(weights['dense_kernel'], stock['dense_kernel']) and np.array_equal(weights['dense_bias'], stock['dense_bias'])

    network = 'restated (oracle/keras_gru.py, make_runner_cls-style class over tests/golden/weights_stock_seed42.npz, through the runner_cls seam)'
    drivers = {
        'generated': ('train_generated.npz', lambda out: drive_generated(ref, wavio, out), 'not used by this fixture (runner_cls=lambda x: None, as the script has it)'),
        'incremental': ('train_incremental.npz', lambda out: drive_incremental(ref, wavio, out, weights), network),
        'sampled': ('train_sampled.npz', lambda out: drive_sampled(ref, out, weights), 'restated (oracle/keras_gru.predict, stock weights): the predictions handed to the script'),
        'simulate': ('simulate.npz', lambda out: drive_simulate(ref, wavio, out, weights), network + '; an empty batch of windows predicts an empty [0, 1] array'),
    }
    for kind in args.only.split(','):
        name, drive, keras_note = drivers[kind]
        out = {}
        glue = drive(out)
        provenance = np.array([
            'glue: reference code, unmodified: ' + glue + '; scripts made with __new__, their own random / glob / Fitipy names rebound, '
            'listener and retrain recorded (tools/make_script_fixtures.py); stub modules: ' + ', '.join(stubbed) + ', wavio (in-memory int16 arrays)',
            'keras: ' + keras_note,
            'sonopy: ' + sonopy_note,
            'numpy: ' + np.__version__,
            'python: %d.%d, PYTHONHASHSEED=0' % sys.version_info[:2],
        ])
        path = os.path.join(args.out, name)
        np.savez_compressed(path, provenance=provenance, **out)
        print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
