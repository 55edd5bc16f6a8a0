"""
Generated training data: the sample stream of ``precise-train-generated`` (scripts/train_generated.py:118-202) on the GPU.

The reference streams every background recording chunk by chunk through a ``Listener``, overlays volume-normalised wake-word
and not-wake-word clips with random gaps on it, and labels each chunk from how much of the last ``buffer_t`` seconds a wake word
covered.  ``Generator`` splits that into a host half and a device half:

    gen = Generator(runner, backgrounds, positives, negatives, chunk_size=2048)
    plan = gen.plan(random.Random(7))               # host, numpy: the script's draws -> segment tables, ids, targets
    gen.load(plan)                                  # device: mix every file, compute every frame once
    mixed = gen.audio(0)                            # float64, what the script's `chunk`s of file 0 concatenate to
    rows = gen.vectorize(plan.ids)                  # float32 [n, n_features, feature_size]
    gen.append_to(trainer, plan.ids, plan.targets)  # ... straight behind the trainer's resident set

``plan`` consumes random draws in exactly the script's lazy order (one per file for the volume, one per clip piece and one per
silence as the chunks need them, and -- ``count_save_draw`` -- the ``random() > 1.0 - save_prob`` the script evaluates for
every emitted sample even at ``save_prob = 0``), so ``random.Random(seed)`` gives the stream the script gives after
``random.seed(seed)``.  Writing debug wavs is not offered.

``replay``: ``chunk_audio_pieces`` (:133-143) keeps ``piece[-(len(piece) % chunk_size):]`` as its leftover, and ``piece`` is a
``(2, n)`` array: ``len(piece)`` is 2 and the leftover is the WHOLE previous piece.  With pieces p0, p1, p2, ... a file sees
chunks(p0), chunks(p0 + p1), chunks(p1 + p2), ...: every piece twice.  ``'reference'`` reproduces that; ``'tail'`` keeps the
unconsumed remainder, which is what the line evidently meant.  Either way the planner flattens the stream into segments and the
device never knows.

Labels (:186-196) come from run lengths over the segment boundaries, not from a materialised ``vals_buffer``; the buffer is
never cleared between files, and neither is the planner's state -- nor the two clip cycles -- between ``plan`` calls.

Reading wav files is left to the caller.  There is no CPU fallback for the device half; ``plan`` needs no GPU.
"""
import math
from collections import deque

import numpy as np

from ._lib import GEN_FILE, GEN_SEGMENT
from .params import pr


def rms(x) -> float:
    """``calc_volume`` (:145-147) on the array ``load_audio`` returns; NaN for an empty array"""
    x = np.asarray(x)
    if x.size == 0:
        return float('nan')
    return math.sqrt(np.mean(np.square(x)))


def label(max_run: int, length: int, last_value) -> int:
    """:189-196 -> 1, 0 or -1 (the chunk is skipped).  A float64 true division against the float64 literals: 19200 / 24000 is
    not > 0.8."""
    p = max_run / length
    if last_value == 0 and p > 0.8:
        return 1
    if p < 0.5:
        return 0
    return -1


class RunLabels:
    """The script's ``vals_buffer`` as runs: ``push(pieces)`` takes one chunk as (value, length) pieces and returns its label.
    The buffer starts as ``buffer_samples`` zeros; ``np.concatenate((vals[len(targets):], targets))`` makes it
    ``max(buffer_samples, chunk)`` long from the first chunk on.  Only the runs of ones inside the window are kept, so a chunk
    costs its pieces plus the runs that leave the window."""

    def __init__(self, buffer_samples: int):
        self.length = int(buffer_samples)
        self.pos = 0                    # values pushed so far
        self.runs = deque()             # [start, end) of every run of ones that still reaches into the window

    def push(self, pieces) -> int:
        n = 0
        last = 0
        for value, length in pieces:
            if length <= 0:
                continue
            if value == 1:
                if self.runs and self.runs[-1][1] == self.pos:
                    self.runs[-1][1] = self.pos + length
                else:
                    self.runs.append([self.pos, self.pos + length])
            self.pos += length
            n += length
            last = value
        self.length = max(self.length, n)
        start = self.pos - self.length
        while self.runs and self.runs[0][1] <= start:
            self.runs.popleft()
        longest = max((end - max(begin, start) for begin, end in self.runs), default=0)
        return label(longest, self.length, last)


class _CountingRng:
    def __init__(self, rng):
        self.rng, self.n = rng, 0

    def random(self):
        self.n += 1
        return self.rng.random()


class Plan:
    """What ``Generator.plan`` returns.  ``files`` (``_lib.GEN_FILE``: background, audio_volume, rms, first_segment,
    n_segments) and ``segments`` (``_lib.GEN_SEGMENT``: clip or -1, first, length, volume, rms, target) are the tables
    ``pe_generator_set_plan`` takes; ``chunk_offsets`` int64 [n_files + 1] the exclusive prefix sum of the files' chunk counts;
    ``ids`` int64 the global chunk ids of the emitted samples in stream order, ``targets`` float32 their 0 / 1 labels;
    ``n_draws`` the random draws consumed; ``replay``, ``chunk_size`` as planned."""

    def __init__(self, files, segments, chunk_offsets, ids, targets, n_draws, replay, chunk_size):
        self.files, self.segments, self.chunk_offsets = files, segments, chunk_offsets
        self.ids, self.targets, self.n_draws, self.replay, self.chunk_size = ids, targets, n_draws, replay, chunk_size

    @property
    def n_chunks(self) -> int:
        return int(self.chunk_offsets[-1])

    def timeline(self, file: int):
        """-> (clip int64 [n], index int64 [n], target int64 [n]) per output sample of planned file ``file``: the clip (-1:
        silence), the sample within it (0 in silence) and the target value under it"""
        f = self.files[file]
        segs = self.segments[int(f['first_segment']):int(f['first_segment'] + f['n_segments'])]
        clip = np.repeat(segs['clip'].astype(np.int64), segs['length'])
        target = np.repeat(segs['target'].astype(np.int64), segs['length'])
        index = np.concatenate([np.arange(s['first'], s['first'] + s['length']) if s['clip'] >= 0 else np.zeros(s['length'], np.int64)
                                for s in segs] or [np.zeros(0, np.int64)])
        return clip, index.astype(np.int64), target


def _named(items, kind):
    """a sequence of arrays, or a dict name -> array -> (names, arrays)"""
    if isinstance(items, dict):
        return [str(k) for k in items], [np.asarray(v) for v in items.values()]
    items = list(items)
    return ['%s[%d]' % (kind, i) for i in range(len(items))], [np.asarray(v) for v in items]


class Generator:
    """``backgrounds``, ``positives``, ``negatives``: sequences of 1-D float32 arrays as ``load_audio`` returns them (or dicts
    name -> array; the names appear in error messages).  ``runner``: a ``HipRunner`` whose engine mixes and vectorizes; it is
    first touched by ``load``, so a planner alone may pass None.  A clip whose rms is 0 or NaN is refused here, by name; a
    background is judged when it is planned (one without a whole chunk is skipped after its volume draw, as the script does)."""

    def __init__(self, runner, backgrounds, positives, negatives, chunk_size: int = 2048, buffer_samples: int = None,
                 sample_rate: int = None):
        self.runner = runner
        self.chunk_size = int(chunk_size)
        if self.chunk_size < 1:
            raise ValueError('chunk_size must be >= 1, got %d' % self.chunk_size)
        self.buffer_samples = int(pr.buffer_samples if buffer_samples is None else buffer_samples)
        self.sample_rate = int(pr.sample_rate if sample_rate is None else sample_rate)
        self.background_names, self.backgrounds = _named(backgrounds, 'backgrounds')
        pos_names, pos = _named(positives, 'positives')
        neg_names, neg = _named(negatives, 'negatives')
        self.clip_names, self.clips = pos_names + neg_names, pos + neg          # one pool: the positives first
        self.n_positives, self.n_negatives = len(pos), len(neg)
        self.background_rms = [rms(a) for a in self.backgrounds]
        self.clip_rms = [rms(a) for a in self.clips]
        for name, v in zip(self.clip_names, self.clip_rms):
            if not v > 0.0:
                raise ValueError('clip %s has rms %r: it cannot be normalised to a volume' % (name, v))
        self._cycle = [0, 0]            # the next negative / positive clip: both cycles persist across files (:115-116)
        self._labels = RunLabels(self.buffer_samples)
        self._g = None

    # -- the host half ------------------------------------------------------------------------------------------------
    def _n_chunks(self, background: int) -> int:
        n = len(self.backgrounds[background])
        return (n - 1) // self.chunk_size if n >= 1 else 0

    def _next_piece(self, rng, pending_silence: bool):
        """generate_wakeword_pieces (:124-131): a clip piece and the silence behind it alternate, one draw each -> (clip, first,
        length, target)"""
        if pending_silence:
            return (-1, 0, int(self.sample_rate * (0.5 + 2.0 * rng.random())), 0)
        target = 1 if rng.random() > 0.5 else 0
        count = self.n_positives if target else self.n_negatives
        if count == 0:
            raise ValueError('the stream asks for a %s clip and there is none' % ('wake-word' if target else 'not-wake-word'))
        k = self._cycle[target] % count
        self._cycle[target] = k + 1
        clip = k if target else self.n_positives + k
        return (clip, 0, len(self.clips[clip]), target)

    @staticmethod
    def _cut(segs, a, b):
        """samples [a, b) of a list of (clip, first, length, target)"""
        out = []
        pos = 0
        for clip, first, length, target in segs:
            lo, hi = max(a, pos), min(b, pos + length)
            if hi > lo:
                out.append((clip, first + (lo - pos) if clip >= 0 else 0, hi - lo, target))
            pos += length
            if pos >= b:
                break
        return out

    def plan(self, rng, files=None, replay: str = 'reference', count_save_draw: bool = True) -> Plan:
        if replay not in ('reference', 'tail'):
            raise ValueError("replay must be 'reference' or 'tail', got %r" % (replay,))
        files = range(len(self.backgrounds)) if files is None else [int(f) for f in files]
        rng = _CountingRng(rng)
        C = self.chunk_size
        file_rows, seg_rows, ids, targets = [], [], [], []
        chunk_offsets = [0]
        for background in files:
            if not 0 <= background < len(self.backgrounds):
                raise ValueError('background %d of %d' % (background, len(self.backgrounds)))
            volume_of = self.background_rms[background]
            audio_volume = volume_of * (0.4 + 0.5 * rng.random())                   # :176-177
            n_chunks = self._n_chunks(background)
            if n_chunks and not volume_of > 0.0:
                raise ValueError('background %s has rms %r: it cannot be normalised to a volume' % (self.background_names[background], volume_of))
            first_segment = len(seg_rows)
            combined, total, at = [], 0, 0                  # the pieces being chunked, their length, the next chunk in them
            previous, pending_silence = None, False
            for i in range(n_chunks):
                while (at + 1) * C >= total:                # chunk_audio: range(C, len, C) -- no chunk ends at len
                    piece = self._next_piece(rng, pending_silence)
                    pending_silence = not pending_silence
                    if replay == 'reference':
                        combined = ([previous] if previous is not None and previous[2] > 0 else []) + [piece]
                    else:
                        combined = self._cut(combined, at * C, total) + [piece]
                    previous = piece
                    total, at = sum(s[2] for s in combined), 0
                chunk = self._cut(combined, at * C, (at + 1) * C)
                at += 1
                for clip, first, length, target in chunk:
                    last = seg_rows[-1] if len(seg_rows) > first_segment else None
                    if last is not None and last[0] == clip and last[5] == target and (clip < 0 or last[1] + last[2] == first):
                        last[2] += length
                    else:
                        seg_rows.append([clip, first, length, audio_volume, self.clip_rms[clip] if clip >= 0 else 0.0, target])
                got = self._labels.push([(t, n) for _, _, n, t in chunk])
                if got >= 0:
                    if count_save_draw:
                        rng.random()                        # :198, evaluated at save_prob = 0 as well
                    ids.append(chunk_offsets[-1] + i)
                    targets.append(got)
            file_rows.append((background, 0, audio_volume, volume_of, first_segment, len(seg_rows) - first_segment))
            chunk_offsets.append(chunk_offsets[-1] + n_chunks)
        segments = np.zeros(len(seg_rows), dtype=GEN_SEGMENT)
        for name, column in zip(('clip', 'first', 'length', 'volume', 'rms', 'target'), zip(*seg_rows)):
            segments[name] = column
        return Plan(np.array(file_rows, dtype=GEN_FILE), segments, np.asarray(chunk_offsets, dtype=np.int64),
                    np.asarray(ids, dtype=np.int64), np.asarray(targets, dtype=np.float32), rng.n, replay, C)

    # -- the device half ----------------------------------------------------------------------------------------------
    def _session(self):
        if self._g is None:
            from ._lib import HipGenerator
            self._g = HipGenerator(self.runner.engine, self.backgrounds, self.clips, self.chunk_size)
        return self._g

    def load(self, plan: Plan):
        """Mix every file of the plan and compute every frame once; the plan stays resident until the next ``load``."""
        if plan.chunk_size != self.chunk_size:
            raise ValueError('the plan was drawn for chunk_size %d, not %d' % (plan.chunk_size, self.chunk_size))
        self._session().set_plan(plan.files, plan.segments)

    def audio(self, file: int, first: int = 0, n: int = None) -> np.ndarray:
        """float64: the mixed samples of planned file ``file`` -- the script's ``chunk``s concatenated"""
        return self._session().audio(file, first, n)

    def vectorize(self, ids) -> np.ndarray:
        """float32 [n, n_features, feature_size]: ``Listener.update_vectors`` after global chunk ``ids[i]`` of the loaded plan, on
        a listener cleared at the start of the file (use_delta: with the delta columns, which the script leaves out)"""
        return self._session().vectorize(ids)

    def append_to(self, trainer, ids, targets, validation: bool = False):
        """The same rows, sample i with ``targets[i]``, behind the trainer's resident training -- or validation -- set,
        without leaving the device."""
        self._session().append(trainer._t, ids, targets, validation=validation)

    def close(self):
        if self._g is not None:
            self._g.close()
            self._g = None
