"""
Noise augmentation: the noisy copies of ``precise-add-noise`` (scripts/add_noise.py:56-90) on the GPU.

The reference makes ``inflation_factor`` copies of every clip of a dataset: a cursor walks through a pool of noise recordings, the
noise under a copy is scaled to the clip's energy (two Python ``sum()`` passes per copy) and mixed in at a random ratio, the
result is saved as an int16 wav, and training reads it back through ``load_audio`` and ``vectorize``.  ``NoiseAugmenter`` splits
that into a host half and a device half:

    aug = NoiseAugmenter(runner, clips, noises, labels)
    plan = aug.plan(random.Random(7), inflation_factor=10)      # host: the cursor and the draws -> copies and pieces
    aug.load(plan)                                              # device: every copy's noise volume
    mixed, saved = aug.audio(0), aug.pcm(0)                     # float64 noised_audio, the int16 save_audio writes
    rows = aug.vectorize()                                      # float32 [n, n_features, feature_size] of the reloaded copies
    aug.append_to(trainer)                                      # ... straight behind the trainer's resident set

``plan`` takes one ``rng.random()`` per copy, in the script's order (clip by clip, then copy by copy), so ``random.Random(seed)``
gives the ratios the script draws after ``random.seed(seed)``.  The noise cursor is ``get_fresh_noise``'s (:66-83) and lives on
across ``plan`` calls, as the script's ``NoiseData`` lives on across clips: a step takes ``src[pos:pos + need]``, adds the whole
``need`` to ``pos`` even when the slice was shorter, and moves on to the next recording -- at position 0 -- as soon as
``pos >= len(src)``, which is also what happens when the slice ended exactly at the end; after the last recording it wraps to the
first and counts a repeat.

Where the reference is undefined: all-zero noise under a copy (its volume is 0, the mix NaN) is refused by ``load``, naming the
copy; a sample whose mix leaves the int16 range is counted (``volumes()``); an empty clip or noise recording is refused here.

Reading and walking folders of wav files is left to the caller (``write_wavs`` writes the copies).  There is no CPU fallback for
the device half; ``plan`` needs no GPU.
"""
import os
import wave

import numpy as np

from ._lib import AUG_COPY, AUG_PIECE
from .generated import _named
from .params import pr


class Plan:
    """What ``NoiseAugmenter.plan`` returns.  ``copies`` (``_lib.AUG_COPY``: clip, ratio, first_piece, n_pieces) and ``pieces``
    (``_lib.AUG_PIECE``: noise, first, length) are the tables ``pe_augmenter_set_plan`` takes: copy ``clip * inflation_factor + k``
    is the k-th copy of clip ``clip``.  ``piece_copy`` int64 and ``piece_start`` int64: the copy of every piece and its first
    output sample there.  ``cursor``: (noise recording, position, repeat count) after the plan; ``n_draws`` the random draws
    consumed; ``inflation_factor`` as planned."""

    def __init__(self, copies, pieces, piece_copy, piece_start, cursor, n_draws, inflation_factor):
        self.copies, self.pieces, self.piece_copy, self.piece_start = copies, pieces, piece_copy, piece_start
        self.cursor, self.n_draws, self.inflation_factor = cursor, n_draws, inflation_factor

    @property
    def n_copies(self) -> int:
        return int(self.copies.size)

    @property
    def clip(self) -> np.ndarray:
        """int64 [n_copies]: the clip of every copy"""
        return self.copies['clip'].astype(np.int64)


class NoiseAugmenter:
    """``clips``, ``noises``: sequences of 1-D float32 arrays as ``load_audio`` returns them (or dicts name -> array; the names
    appear in error messages).  ``labels``: one target in [0, 1] per clip, the default targets of ``append_to``.  ``runner``: a
    ``HipRunner`` whose engine mixes and vectorizes; it is first touched by ``load``, so a planner alone may pass None."""

    def __init__(self, runner, clips, noises, labels=None):
        self.runner = runner
        self.clip_names, self.clips = _named(clips, 'clips')
        self.noise_names, self.noises = _named(noises, 'noises')
        if not self.clips:
            raise ValueError('no clips to augment')
        if not self.noises:
            raise ValueError('no noise recordings')
        for kind, names, arrays in (('clip', self.clip_names, self.clips), ('noise recording', self.noise_names, self.noises)):
            for name, a in zip(names, arrays):
                if a.ndim != 1 or a.dtype != np.float32:
                    raise ValueError('%s %s must be a 1-D float32 array (load_audio), got %s %r' % (kind, name, a.dtype, a.shape))
                if a.size == 0:
                    raise ValueError('%s %s is empty' % (kind, name))
        self.labels = None
        if labels is not None:
            self.labels = np.ascontiguousarray(labels, dtype=np.float32).reshape(-1)
            if self.labels.size != len(self.clips):
                raise ValueError('%d labels for %d clips' % (self.labels.size, len(self.clips)))
        self.noise_id, self.noise_pos, self.repeat_count = 0, 0, 0      # NoiseData's cursor (:62-64)
        self._plan = None
        self._g = None

    # -- the host half ------------------------------------------------------------------------------------------------
    def _fresh_noise(self, n: int):
        """get_fresh_noise(n) (:66-83) as pieces -> [(noise recording, first sample, length)]"""
        out, have = [], 0
        while have < n:
            size = len(self.noises[self.noise_id])
            need = n - have
            took = min(self.noise_pos + need, size) - self.noise_pos        # len(src[pos:pos + need]); pos < size always
            out.append((self.noise_id, self.noise_pos, took))
            self.noise_pos += need
            if self.noise_pos >= size:
                self.noise_pos = 0
                self.noise_id += 1
                if self.noise_id >= len(self.noises):
                    self.noise_id = 0
                    self.repeat_count += 1
            have += took
        return out

    def plan(self, rng, inflation_factor: int = 1, ratio_low: float = 0.0, ratio_high: float = 0.4) -> Plan:
        inflation_factor = int(inflation_factor)
        if inflation_factor < 0:
            raise ValueError('inflation_factor must be >= 0, got %d' % inflation_factor)
        low, high = float(ratio_low), float(ratio_high)
        copy_rows, piece_rows, piece_copy, piece_start = [], [], [], []
        n_draws = 0
        for clip, audio in enumerate(self.clips):
            for _ in range(inflation_factor):
                ratio = low + (high - low) * rng.random()                   # :123, in double
                n_draws += 1
                pieces = self._fresh_noise(len(audio))
                copy_rows.append((clip, 0, ratio, len(piece_rows), len(pieces)))
                start = 0
                for noise, first, length in pieces:
                    piece_rows.append((noise, 0, first, length))
                    piece_copy.append(len(copy_rows) - 1)
                    piece_start.append(start)
                    start += length
        return Plan(np.array(copy_rows, dtype=AUG_COPY), np.array(piece_rows, dtype=AUG_PIECE), np.asarray(piece_copy, dtype=np.int64),
                    np.asarray(piece_start, dtype=np.int64), (self.noise_id, self.noise_pos, self.repeat_count), n_draws, inflation_factor)

    # -- the device half ----------------------------------------------------------------------------------------------
    def _session(self):
        if self._g is None:
            from ._lib import HipAugmenter
            self._g = HipAugmenter(self.runner.engine, self.clips, self.noises)
        return self._g

    def load(self, plan: Plan):
        """Compute the noise volume of every copy of the plan; the plan stays resident until the next ``load`` that succeeds.  A
        copy over all-zero noise is a ValueError naming the copy, and the plan that was resident stays."""
        self._session().set_plan(plan.copies, plan.pieces)
        self._plan = plan

    def _loaded(self) -> Plan:
        if self._plan is None:
            raise ValueError('no plan is loaded')
        return self._plan

    def volumes(self):
        """-> (float64 [n_clips] ``audio_volume`` of every clip, float64 [n_copies] ``noise_volume`` of every copy of the loaded
        plan, int64 [n_copies] ``overflowed``: the samples of the copy whose mix leaves the int16 range when it is saved)"""
        self._loaded()
        return self._session().volumes()

    def audio(self, copy: int) -> np.ndarray:
        """float64: what ``noised_audio`` returns for copy ``copy`` of the loaded plan"""
        self._loaded()
        return self._session().audio(copy)

    def pcm(self, copy: int) -> np.ndarray:
        """int16: what ``save_audio`` writes for it"""
        self._loaded()
        return self._session().pcm(copy)

    def vectorize(self, ids=None) -> np.ndarray:
        """float32 [n, n_features, feature_size]: ``vectorize`` (``vectorize_delta`` with use_delta) of copies ``ids`` (default:
        all, in order) as ``load_audio`` reads them back, rounded to float32 as the trainer holds them"""
        self._loaded()
        return self._session().vectorize(ids, pr.max_samples)

    def append_to(self, trainer, ids=None, targets=None, validation: bool = False):
        """The same rows behind the trainer's resident training -- or validation -- set, without leaving the device.  ``targets``
        default to the label of each copy's clip."""
        plan = self._loaded()
        ids = np.arange(plan.n_copies) if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)
        if targets is None:
            if self.labels is None:
                raise ValueError('no targets given and the augmenter has no labels')
            if ids.size and (ids.min() < 0 or ids.max() >= plan.n_copies):
                raise ValueError('copy ids must be in 0..%d' % (plan.n_copies - 1))
            targets = self.labels[plan.clip[ids]]
        self._session().append(trainer._t, ids, targets, validation=validation, max_samples=pr.max_samples)

    def write_wavs(self, folder: str, names):
        """One 16-bit mono wav per copy of the loaded plan, ``names[copy]`` under ``folder``: the int16 the reference saves."""
        plan = self._loaded()
        names = list(names)
        if len(names) != plan.n_copies:
            raise ValueError('%d names for %d copies' % (len(names), plan.n_copies))
        for copy, name in enumerate(names):
            path = os.path.join(folder, name)
            os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
            with wave.open(path, 'wb') as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(pr.sample_rate)
                w.writeframes(self.pcm(copy).astype('<i2').tobytes())

    def close(self):
        if self._g is not None:
            self._g.close()
            self._g = None
