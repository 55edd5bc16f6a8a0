"""
Mining false activations: the scan of ``precise-train-incremental`` (scripts/train_incremental.py:113-137) on the GPU.

The reference plays hours of not-wake-word recordings through a live ``Listener``, one ``update`` per chunk, and saves the last
``buffer_t`` seconds whenever the model fires.  ``Miner`` holds the recordings on the device, computes their frames once, and

    miner = Miner(runner, audios, chunk_size=2048)
    hits, n_above, _ = miner.scan(first=0, threshold=0.5)       # every chunk from `first` on, in a few launches
    recording, chunk = miner.locate(hits)
    rows = miner.vectorize(hits)                                # what vectorize(load_audio(saved wav)) would give
    miner.append_to(trainer, hits)                              # ... straight into the trainer's resident set

A chunk's prediction is, bit for bit, what a ``Listener`` cleared at the start of the recording returns for it when it is fed
float samples (``update_raw``); a hit's rows are ``vectorize`` of the script's ring after save_audio / load_audio's int16 round
trip.  Chunks carry GLOBAL ids: recording r's chunk i is ``chunk_offsets[r] + i`` (``chunk_audio``: a recording of ``len``
samples has ``(len - 1) // chunk_size`` chunks).  ``train.IncrementalTrainer`` is the script's policy on top of this.

Reading wav files is left to the caller, as in ``simulate.py``.  There is no CPU fallback.
"""
import numpy as np

from ._lib import HipMiner
from .params import pr


class Miner:
    """``runner``: a ``HipRunner`` (its engine scores the chunks; ``runner.set_weights`` changes what the next scan sees).
    ``audios``: a sequence of 1-D sample arrays (float32 as ``load_audio`` returns them, or float64); empty ones are allowed.
    ``carry_audio``: True = the script's ring, which is never cleared between recordings (train_incremental.py:79,123); False =
    zeros before each recording's own start."""

    def __init__(self, runner, audios, chunk_size: int = 2048, carry_audio: bool = True, buffer_samples: int = None):
        self.runner = runner
        self.chunk_size = int(chunk_size)
        self.buffer_samples = int(pr.buffer_samples if buffer_samples is None else buffer_samples)
        if self.buffer_samples > pr.max_samples:        # vectorize() would crop the saved clip and anchor its frames anew
            raise ValueError('buffer_samples = %d exceeds max_samples = %d' % (self.buffer_samples, pr.max_samples))
        self._m = HipMiner(runner.engine, audios, self.chunk_size, self.buffer_samples, carry_audio)

    @property
    def chunk_offsets(self) -> np.ndarray:
        """int64 [n_recordings + 1]: the exclusive prefix sum of the recordings' chunk counts"""
        return self._m.chunk_offsets

    @property
    def n_chunks(self) -> int:
        return self._m.n_chunks

    def scan(self, first: int = 0, threshold: float = 0.5, capacity: int = None, return_scores: bool = False, model: int = 0):
        """The chunks ``first .. n_chunks`` judged by the runner's network as it is now.  -> (hits, n_above, scores): the
        ascending global ids of the first ``capacity`` chunks with ``decode(p) > threshold`` (float64, strict; ``decode`` is the
        engine's ThresholdDecoder table when ``engine.set_decoder`` was called, else the prediction itself), the number of
        all such chunks in the range, and -- ``return_scores`` -- the raw predictions float32 [n_chunks - first]."""
        return self._m.scan(first, threshold, capacity, return_scores, model)

    def locate(self, hits):
        """global chunk ids -> (recording, chunk within the recording), two int64 arrays"""
        hits = np.asarray(hits, dtype=np.int64).reshape(-1)
        rec = np.searchsorted(self.chunk_offsets, hits, side='right') - 1
        return rec, hits - self.chunk_offsets[rec]

    def vectorize(self, hits) -> np.ndarray:
        """float64 [n, n_features, n_mfcc]: per hit ``vectorize`` of the saved ring (train_incremental.py:130, util.py:65,71)"""
        return self._m.vectorize(hits)

    def append_to(self, trainer, hits, validation: bool = False):
        """The same rows as float32 (use_delta: with their delta columns) behind the trainer's resident training -- or
        validation -- set, target 0, without leaving the device."""
        self._m.append(trainer._t, hits, validation=validation, target=0.0)

    def close(self):
        self._m.close()
