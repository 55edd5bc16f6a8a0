"""What precise-add-noise does with its audio, restated with numpy and builtin sum (not a test; imported by test_augment*.py
and tools/bench_augment.py).  The slow, obviously-right version: the planner and the device are held to it.

Written from the script's contract (scripts/add_noise.py:56-90,118-127, util.py:65,71):
  * the noise pool keeps a cursor (recording, position) and a repeat count for as long as the script runs;
  * fresh noise of n samples starts as np.empty(0) -- float64 -- and is grown by np.concatenate: a step slices the current
    recording from the position over what is still missing, adds ALL that was missing to the position whether or not the slice
    was that long, and when the position has reached or passed the recording's length resets it to 0 and goes to the next
    recording, wrapping to the first one with repeat count + 1;
  * the volumes are sqrt(sum(x ** 2)) with Python's builtin sum: over the float32 clip a float32 chain, over the float64 noise a
    float64 chain, both left to right from the int 0;
  * adjusted noise = clip volume * noise / noise volume, mix = ratio * adjusted noise + (1.0 - ratio) * clip: the Python float
    meets the float32 clip as a float32, everything else is float64;
  * per clip, in order, inflation_factor copies, each with the ratio low + (high - low) * random();
  * saved as (mix * 32767).astype(int16); loaded as int16.astype(float32) / 32767.0.
"""
import math

import numpy as np


class Pool:
    """the noise recordings and the cursor into them"""

    def __init__(self, recordings):
        self.recordings = list(recordings)
        self.index = 0
        self.position = 0
        self.repeats = 0

    @property
    def cursor(self):
        return (self.index, self.position, self.repeats)

    def fresh(self, n):
        got = np.empty(0)
        self.last_steps = []                # (recording, position, slice length) of every step: for the planner's tests
        while len(got) < n:
            source = self.recordings[self.index]
            missing = n - len(got)
            part = source[self.position:self.position + missing]
            self.last_steps.append((self.index, self.position, len(part)))
            self.position += missing
            if self.position >= len(source):
                self.position = 0
                self.index += 1
                if self.index >= len(self.recordings):
                    self.index = 0
                    self.repeats += 1
            got = np.concatenate([got, part])
        return got

    def mix(self, clip, ratio):
        """-> (mix float64, clip volume, noise volume)"""
        noise = self.fresh(len(clip))
        clip_volume = math.sqrt(sum(clip ** 2))
        noise_volume = math.sqrt(sum(noise ** 2))
        adjusted = clip_volume * noise / noise_volume
        return ratio * adjusted + (1.0 - ratio) * clip, clip_volume, noise_volume


def saved(mix):
    return (mix * np.iinfo(np.int16).max).astype(np.int16)


def loaded(pcm):
    return pcm.astype(np.float32) / float(np.iinfo(pcm.dtype).max)


def out_of_range(mix):
    """samples save_audio cannot represent: the cast of |mix * 32767| >= 32768 to int16 is undefined"""
    scaled = mix * np.iinfo(np.int16).max
    return int(np.count_nonzero(~((scaled > -32768.0) & (scaled < 32768.0))))


class Copy:
    def __init__(self, clip, ratio, mix, clip_volume, noise_volume, steps, cursor):
        self.clip, self.ratio, self.mix, self.clip_volume, self.noise_volume = clip, ratio, mix, clip_volume, noise_volume
        self.steps, self.cursor = steps, cursor


def run(clips, pool, rng, inflation_factor=1, low=0.0, high=0.4):
    """the script's two loops over loaded clips -> [Copy] in the order the script writes its files"""
    copies = []
    for c, clip in enumerate(clips):
        for _ in range(inflation_factor):
            ratio = low + (high - low) * rng.random()
            with np.errstate(all='ignore'):
                mix, va, vn = pool.mix(clip, ratio)
            copies.append(Copy(c, ratio, mix, va, vn, pool.last_steps, pool.cursor))
    return copies


class CountingRng:
    def __init__(self, rng):
        self.rng, self.n = rng, 0

    def random(self):
        self.n += 1
        return self.rng.random()
