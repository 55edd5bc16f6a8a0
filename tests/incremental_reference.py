"""What precise-train-incremental does with its audio, restated in numpy (not a test; imported by test_mining*.py).

Written from the script's contract (scripts/train_incremental.py:113-137, util.py:30-32,45-72):
  * chunk i of a recording is samples [i C, (i + 1) C) for (i + 1) C < len: (len - 1) // C chunks, 0 for an empty recording;
  * a float64 ring of buffer_samples samples starts as zeros, takes every chunk and is never cleared between recordings;
  * a saved ring goes through int16: q = (x * 32767.0).astype(int16) (truncation toward zero), y = float32(q) / float32(32767);
  * per recording a flag says whether its hits go to the test set; after EVERY chunk `not test and count >= delay_samples and
    epochs > 0` retrains and resets the count; hits of test recordings count but never trigger.

Held in turn to the script itself: tests/golden/train_incremental.npz is what the reference's own
``TrainIncrementalScript.train_on_audio`` did over four recordings on one script object (tools/make_script_fixtures.py), and
test_mining_host.py asks ``policy_loop``, ``rings`` and ``saved_pcm`` for the same hits, saved int16 rings and retrain points --
and that ``rings(..., carry_audio=False)`` does NOT give them.
"""
import numpy as np


def n_chunks(length: int, chunk_size: int) -> int:
    return (length - 1) // chunk_size if length >= 1 else 0


def chunk_offsets(lengths, chunk_size: int) -> np.ndarray:
    out = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum([n_chunks(int(n), chunk_size) for n in lengths], out=out[1:])
    return out


def chunks(audio, chunk_size: int):
    for end in range(chunk_size, len(audio), chunk_size):
        yield audio[end - chunk_size:end]


def saved_pcm(ring) -> np.ndarray:
    """save_audio: the int16 samples a float64 ring is written as"""
    return (np.asarray(ring, dtype=np.float64) * 32767.0).astype(np.int16)


def round_trip(ring) -> np.ndarray:
    """save_audio then load_audio: float64 ring -> float32 samples"""
    return saved_pcm(ring).astype(np.float32) / np.float32(32767.0)


def rings(audios, chunk_size: int, buffer_samples: int, carry_audio: bool = True, only=None) -> list:
    """the float64 ring after every chunk of every recording, in global chunk order (before the int16 round trip); with
    ``only`` (a set of global chunk ids) the other entries are None: a session of many chunks keeps the rings it compares"""
    out = []
    ring = np.zeros(buffer_samples, dtype=np.float64)
    for audio in audios:
        if not carry_audio:
            ring = np.zeros(buffer_samples, dtype=np.float64)
        for chunk in chunks(np.asarray(audio), chunk_size):
            ring = np.concatenate((ring[len(chunk):], chunk))[-buffer_samples:]
            out.append(ring if only is None or len(out) in only else None)
    return out


def locate(lengths, chunk_size: int) -> list:
    """(recording, chunk within the recording) of every global chunk id, by the loop the script runs"""
    return [(r, i) for r, n in enumerate(lengths) for i in range(n_chunks(int(n), chunk_size))]


def emitted_frames(n_samples, window_samples: int, hop_samples: int) -> np.ndarray:
    """frames a Listener cleared at the recording's start has emitted once n samples have arrived (network_runner.py:137-144:
    vectorize_raw of everything buffered returns 1 + (len - window) // hop frames and leaves the rest; nothing below one window)"""
    n = np.asarray(n_samples, dtype=np.int64)
    return np.where(n >= window_samples, 1 + (n - window_samples) // hop_samples, 0)


def policy_loop(audios, test_flags, chunk_size, buffer_samples, delay_samples, epochs, threshold, start_recording, predict, retrain,
                count=0):
    """The script's loop.  ``start_recording(r)`` is Listener.clear; ``predict(r, i, chunk)`` the confidence of chunk i of
    recording r; ``retrain(saved)`` runs when the policy fires, with every saved sample so far as (round-tripped ring, test).
    -> (hits [(recording, chunk, test)], retrains [(recording, chunk)], saved, count)"""
    ring = np.zeros(buffer_samples, dtype=np.float64)
    hits, retrains, saved = [], [], []
    for r, audio in enumerate(audios):
        test = bool(test_flags[r])
        start_recording(r)
        for i, chunk in enumerate(chunks(np.asarray(audio), chunk_size)):
            ring = np.concatenate((ring[len(chunk):], chunk))[-buffer_samples:]
            if float(predict(r, i, chunk)) > threshold:
                count += 1
                hits.append((r, i, test))
                saved.append((round_trip(ring), test))
            if not test and count >= delay_samples and epochs > 0:
                count = 0
                retrains.append((r, i))
                retrain(saved)
    return hits, retrains, saved, count


def fixture_recordings(g):
    """the fixture's int16 recordings as load_audio returns them"""
    off = g['offsets']
    return [g['pcm'][a:b].astype(np.float32) / float(np.iinfo(np.int16).max) for a, b in zip(off[:-1], off[1:])]
