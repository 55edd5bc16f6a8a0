"""What precise-train-generated does with its audio, restated with numpy and real generators (not a test; imported by
test_generated*.py).  The slow, obviously-right version: the planner and the device are held to it.

Held in turn to the script itself: tests/golden/train_generated.npz is what the reference's own
``TrainGeneratedScript.vectors_from_fn`` gave over five background files on one script object (tools/make_script_fixtures.py),
and test_generated_host.py asks this restatement for the same labels, draws per file, clips pulled, run summaries, merged audio
bits and emitted windows -- and that ``mode='tail'`` and ``save_draw=False`` do NOT give them.

Written from the script's contract (scripts/train_generated.py:118-202, util.py:30-32):
  * a file's volume is rms(audio) * (0.4 + 0.5 * random()); audio and every clip are scaled `volume * x / rms(x)`, which is
    float32 arithmetic on the float32 arrays load_audio returns;
  * the wake-word stream is an endless generator: draw a target (random() > 0.5), take the next clip of the positive or the
    negative cycle (both cycles live as long as the script), yield it as a (2, n) float64 array [samples; target], then yield
    int(sample_rate * (0.5 + 2.0 * random())) zeros with target 0 -- each draw happens when the piece is pulled;
  * the pieces are cut into chunks by concatenating a leftover in front of each piece and taking the (len - 1) // C whole
    chunks; the leftover is `piece[-(len(piece) % C):]` with len(piece) == 2 (the number of ROWS): the whole piece.  mode
    'tail' keeps the columns that were not consumed instead;
  * zip(background chunks, wake-word chunks): the background is asked first, so a file that ends pulls nothing more;
  * chunk = (1.0 - 0.6) * bg + 0.6 * ww: a float32 product plus a float64 product;
  * vals_buffer (buffer_samples zeros at the start, never cleared) takes every chunk's targets; p = longest run of ones / its
    length; target 1 if its last value is 0 and p > 0.8, target 0 if p < 0.5, else the chunk yields nothing;
  * before an emitted sample is yielded, `random() > 1.0 - save_prob` is evaluated: one more draw (save_draw).
"""
import math
import random
from itertools import cycle

import numpy as np


def calc_volume(sample):
    return math.sqrt(np.mean(np.square(sample)))


def normalize_volume_to(sample, volume):
    return volume * sample / calc_volume(sample)


def layer_with(sample, value):
    b = np.full((2, len(sample)), value, dtype=float)
    b[0] = sample
    return b


def chunk_audio(audio, chunk_size):
    for i in range(chunk_size, len(audio), chunk_size):
        yield audio[i - chunk_size:i]


def merge(a, b, ratio):
    return (1.0 - ratio) * a + ratio * b


def max_run_length(x, val):
    if x.size == 0:
        return 0
    y = np.array(x[1:] != x[:-1])
    i = np.append(np.where(y), len(x) - 1)
    run_lengths = np.diff(np.append(-1, i))
    run_length_values = x[i]
    return max([rl for rl, v in zip(run_lengths, run_length_values) if v == val], default=0)


def literal_label(vals):
    """-> 1, 0 or -1 (no sample) from the materialised buffer"""
    percent_overlapping = max_run_length(vals, 1) / len(vals)
    if vals[-1] == 0 and percent_overlapping > 0.8:
        return 1
    if percent_overlapping < 0.5:
        return 0
    return -1


class CountingRng:
    """``random()`` from a scripted list of draws (or any object with .random()), counting the calls"""

    def __init__(self, draws):
        self.draws = iter(draws) if isinstance(draws, (list, tuple)) else None
        self.rng = None if self.draws is not None else draws
        self.n = 0

    def random(self):
        self.n += 1
        return next(self.draws) if self.draws is not None else self.rng.random()


class Script:
    """The state the script keeps between files: the two clip cycles, vals_buffer, the random generator."""

    def __init__(self, positives, negatives, rng, chunk_size, buffer_samples, sample_rate=16000, mode='reference', save_draw=True):
        self.positives, self.negatives = list(positives), list(negatives)
        # the cycles yield (index in the pool of positives followed by negatives, samples)
        self.pos_it = iter(cycle([(i, c) for i, c in enumerate(self.positives)]))
        self.neg_it = iter(cycle([(len(self.positives) + i, c) for i, c in enumerate(self.negatives)]))
        self.rng, self.chunk_size, self.sample_rate, self.mode, self.save_draw = rng, chunk_size, sample_rate, mode, save_draw
        self.vals_buffer = np.zeros(buffer_samples, dtype=float)
        self.taken = []             # pool index of every clip pulled, in order

    def wakeword_sample(self, index, clip, volume):
        """row 0 of a clip piece (test_generated_host.py overrides this to follow where every sample comes from)"""
        return normalize_volume_to(clip, volume)

    def generate_wakeword_pieces(self, volume):
        while True:
            target = 1 if self.rng.random() > 0.5 else 0
            it = self.pos_it if target else self.neg_it
            index, clip = next(it)
            self.taken.append(index)
            yield layer_with(self.wakeword_sample(index, clip, volume), target)
            yield layer_with(np.zeros(int(self.sample_rate * (0.5 + 2.0 * self.rng.random()))), 0)

    def chunk_audio_pieces(self, pieces, chunk_size):
        left_over = np.array([])
        for piece in pieces:
            if left_over.size == 0:
                combined = piece
            else:
                combined = np.concatenate([left_over, piece], axis=-1)
            consumed = 0
            for chunk in chunk_audio(combined.T, chunk_size):
                consumed += chunk_size
                yield chunk.T
            if self.mode == 'reference':
                left_over = piece[-(len(piece) % chunk_size):]
            else:
                left_over = combined[:, consumed:]

    def vectors_from(self, audio):
        """one background file -> per chunk (i, chunk float64, chunk_ww, targets, label); label -1: the script yields nothing"""
        audio_volume = calc_volume(audio) if len(audio) else float('nan')
        audio_volume *= 0.4 + 0.5 * self.rng.random()
        with np.errstate(all='ignore'):
            audio = normalize_volume_to(audio, audio_volume) if len(audio) else audio
        chunked_bg = chunk_audio(audio, self.chunk_size)
        chunked_ww = self.chunk_audio_pieces(self.generate_wakeword_pieces(audio_volume), self.chunk_size)
        for i, (chunk_bg, (chunk_ww, targets)) in enumerate(zip(chunked_bg, chunked_ww)):
            chunk = merge(chunk_bg, chunk_ww, 0.6)
            self.vals_buffer = np.concatenate((self.vals_buffer[len(targets):], targets))
            got = literal_label(self.vals_buffer)
            if got >= 0 and self.save_draw:
                self.rng.random()
            yield i, chunk, chunk_ww, targets, got


def run(backgrounds, positives, negatives, draws, chunk_size, buffer_samples, sample_rate=16000, mode='reference', save_draw=True,
        script_cls=Script):
    """every file in order -> (per file the list of vectors_from's tuples, the script with its state, draws consumed)"""
    rng = CountingRng(draws)
    script = script_cls(positives, negatives, rng, chunk_size, buffer_samples, sample_rate, mode, save_draw)
    return [list(script.vectors_from(np.asarray(a))) for a in backgrounds], script, rng.n


# ---- the inputs both test files use ----------------------------------------------------------------------------------------
B = 24000           # ListenerParams.buffer_samples of the stock parameters
LONG_CLIP = 23200   # > 0.8 * 24000: a wake word long enough for a target 1


def tone(seed, n):
    """float32 samples in (-1, 1) as load_audio returns them: k / 32767"""
    k = np.random.default_rng(seed).integers(-20000, 20000, n)
    return (k.astype(np.float32) / np.float32(32767.0)).astype(np.float32)


def inputs(C):
    """backgrounds (the long one first: the scripted draws open it), positives, negatives"""
    backgrounds = [tone(s, n) for s, n in enumerate([47000, 0, 1, C, C + 1, 2 * C + 1, 47000])]
    positives = [tone(10, LONG_CLIP), tone(11, 1), tone(12, C)]
    negatives = [tone(20, C - 1), tone(21, 2 * C + 1)]
    return backgrounds, positives, negatives


def draws():
    """file 0: u = 0.37 for the volume (its float32 rounding matters), a positive (the 23 200-sample clip), its silence of
    int(16000 * 0.7) samples; then a fixed pseudo-random tail"""
    tail = random.Random(5)
    return [0.37, 0.9, 0.1] + [tail.random() for _ in range(4000)]


# ---- the script's own stream: tests/golden/train_generated.npz ----------------------------------------------------------------
def fixture_pools(g, C):
    """the fixture's int16 pools as load_audio returns them -> (backgrounds, positives, negatives, draws)"""
    k = '_%d' % C
    cut = lambda pcm, off: [pcm[a:b].astype(np.float32) / float(np.iinfo(np.int16).max) for a, b in zip(off[:-1], off[1:])]
    clips = cut(g['clip_pcm' + k], g['clip_offsets' + k])
    n_pos = int(g['n_positives' + k])
    return cut(g['background_pcm' + k], g['background_offsets' + k]), clips[:n_pos], clips[n_pos:], g['draws' + k].tolist()
