#!/usr/bin/env python3
"""
Write tests/golden/add_noise.npz: what the reference's own ``NoiseData`` (precise/scripts/add_noise.py) and its own
``load_audio`` / ``save_audio`` (precise/util.py) compute for a small seeded dataset.

    python tools/make_add_noise_fixture.py --reference /path/to/mycroft-precise

The script module imports packages it never uses on this path (prettyparse, pyache, fitipy, sonopy, speechpy) and ``wavio``,
which load_audio / save_audio use only to move int16 arrays in and out of files.  None of them has to be installed: the first
group is replaced by empty stub modules, and ``wavio`` by an in-memory stand-in that hands load_audio the int16 array it was
asked for and keeps the int16 array save_audio hands it.  Everything between those two points is the reference's code, unmodified.

Contents: ``clip_pcm`` / ``clip_offsets`` and ``noise_pcm`` / ``noise_offsets`` (int16 pools), ``inflation_factor``, per copy in the
script's order ``clip``, ``ratio``, ``cursor`` (noise_data_id, noise_pos, repeat_count after the call) and, concatenated,
``mixed`` (float64, noised_audio's result) and ``saved`` (int16, what save_audio wrote).  Amplitudes stay below 8000 / 32767, which
keeps every mix far inside the int16 range (asserted here).
"""
import argparse
import os
import random
import sys

import numpy as np

from reference_stubs import install_stubs, install_wavio

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'add_noise.npz')

# (no length 1: load_audio squeezes a one-sample wav to a 0-d array, which the script cannot slice or measure)
CLIP_LENGTHS = (2, 65, 300, 700, 1300)
NOISE_LENGTHS = (2, 300, 700, 1000)
INFLATION = 2
AMPLITUDE = 8000


def pcm(rng, n):
    """a tone plus noise, int16, |x| <= AMPLITUDE"""
    t = np.arange(n)
    x = 0.6 * np.sin(2 * np.pi * t * rng.uniform(0.01, 0.2)) + 0.4 * rng.uniform(-1.0, 1.0, n)
    return np.round(AMPLITUDE * x).astype(np.int16)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', required=True, help='a checkout of the reference implementation')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()

    stubbed = install_stubs(('prettyparse', 'pyache', 'fitipy', 'sonopy', 'speechpy'))
    sys.path.insert(0, os.path.abspath(args.reference))
    from precise.params import pr
    wavio = install_wavio(pr.sample_rate)
    stubbed.append('wavio (in-memory int16 arrays)')
    from precise.scripts import add_noise
    from precise.util import load_audio, save_audio

    rng = np.random.default_rng(20260118)
    clip_pcm = [pcm(rng, n) for n in CLIP_LENGTHS]
    noise_pcm = [pcm(rng, n) for n in NOISE_LENGTHS]
    for i, a in enumerate(clip_pcm):
        wavio.files['clip%d' % i] = a
    for i, a in enumerate(noise_pcm):
        wavio.files['noise%d' % i] = a

    noise_data = add_noise.NoiseData.__new__(add_noise.NoiseData)         # its __init__ globs a folder; the rest is as written
    noise_data.noise_data = [load_audio('noise%d' % i) for i in range(len(noise_pcm))]
    noise_data.noise_data_id, noise_data.noise_pos, noise_data.repeat_count = 0, 0, 0

    draws = random.Random(7)
    clip, ratio, cursor, mixed, saved = [], [], [], [], []
    for c in range(len(clip_pcm)):
        audio = load_audio('clip%d' % c)
        assert audio.dtype == np.float32
        for k in range(INFLATION):
            r = 0.0 + (0.4 - 0.0) * draws.random()
            altered = noise_data.noised_audio(audio, r)
            assert altered.dtype == np.float64 and np.all(np.abs(altered) < 0.25)
            save_audio('out', altered)
            clip.append(c)
            ratio.append(r)
            cursor.append((noise_data.noise_data_id, noise_data.noise_pos, noise_data.repeat_count))
            mixed.append(altered)
            saved.append(wavio.files['out'])

    def offsets(arrays):
        return np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)

    provenance = np.array([
        'glue: reference code, unmodified: precise/scripts/add_noise.py (NoiseData.get_fresh_noise, NoiseData.noised_audio), '
        'precise/util.py (load_audio, save_audio); stub modules: ' + ', '.join(stubbed),
        'keras: not used by this fixture',
        'sonopy: not used by this fixture',
        'numpy: ' + np.__version__,
        'python: %d.%d' % sys.version_info[:2],
    ])
    np.savez_compressed(args.out, provenance=provenance, clip_pcm=np.concatenate(clip_pcm), clip_offsets=offsets(clip_pcm),
                        noise_pcm=np.concatenate(noise_pcm), noise_offsets=offsets(noise_pcm), inflation_factor=np.int64(INFLATION),
                        seed=np.int64(7), clip=np.array(clip, dtype=np.int64), ratio=np.array(ratio, dtype=np.float64),
                        cursor=np.array(cursor, dtype=np.int64), mixed=np.concatenate(mixed), saved=np.concatenate(saved))
    print(args.out, os.path.getsize(args.out), 'bytes;', len(clip), 'copies; final cursor', cursor[-1])


if __name__ == '__main__':
    main()
