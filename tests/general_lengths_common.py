"""Plain Python, no GPU: what tests/test_general_lengths.py and tests/test_general_lengths_host.py share.

The general front end (csrc/mfcc_general_device.h) is ELEVEN transform instantiations (kernels.hip: with_general_bits),
each in float64 and float32 and in four kernels (stream, offline, clips, recs):

    packed real FFT   BITS 5 .. 10   n_fft 64, 128, 256, 512, 1024, 2048          (BITS = log2(n_fft / 2))
    Bluestein         BITS 7 .. 11   L = 128 .. 2048 = next_pow2(2 n_fft - 1)     every other n_fft in 16 .. 1024

``LENGTHS`` holds at least one parameter set per instantiation, and for Bluestein the n_fft at both ends of every
length: the tightest fits 63, 127, 255, 511, 1023 (2 N - 1 is 3 below L) and the loosest 65, 129, 257, 513.
``instantiation`` restates the launchers' dispatch so that the host test can show the table covers all eleven.

``float32_restatement`` is the oracle's pipeline (oracle/sonopy_restated.py, Q1-Q7) with every array float32.  It is the
measuring stick of the float32 kernels' rounding error, not a second oracle: the float32 kernels are held to the float64
oracle, and their distance from it is compared with the distance this restatement keeps on the same frames."""
import numpy as np
import scipy.fft
from scipy.fftpack import dct

from mycroft_precise_amd import synth
from oracle import sonopy_restated as sr

N_SAMPLES = 20000           # offline buffers


def _set(n_fft, n_filt, n_mfcc, **kw):
    return dict(n_fft=n_fft, n_filt=n_filt, n_mfcc=n_mfcc, **kw)


# (form, BITS) -> parameter sets; stock window_t / hop_t / buffer_t (1600 / 800 samples, 29 frames) unless said otherwise
TABLE = {
    ('pow2', 5): [_set(64, 8, 6)],
    ('pow2', 6): [_set(128, 12, 8)],
    ('pow2', 7): [_set(256, 20, 13)],
    ('pow2', 8): [_set(512, 80, 32)],
    ('pow2', 9): [_set(1024, 40, 20)],
    ('pow2', 10): [_set(2048, 30, 13)],
    ('blue', 7): [_set(17, 4, 4), _set(63, 8, 6)],
    ('blue', 8): [_set(65, 8, 6), _set(127, 12, 8),
                  _set(96, 10, 8, window_t=0.005, hop_t=0.0025, buffer_t=0.2)],       # window (80) < n_fft: zero-padded frames
    ('blue', 9): [_set(129, 12, 8), _set(160, 16, 13), _set(255, 20, 13)],
    ('blue', 10): [_set(257, 20, 13), _set(511, 20, 13)],
    ('blue', 11): [_set(513, 20, 13), _set(1023, 40, 20)],
}
LENGTHS = [kw for sets in TABLE.values() for kw in sets]
TIGHTEST = (63, 127, 255, 511, 1023)        # 2 N - 1 = L - 3
LOOSEST = (65, 129, 257, 513)               # 2 N - 1 = L / 2 + 1: the first n_fft of the next length


def set_id(kw):
    return 'fft%d_filt%d_mfcc%d' % (kw['n_fft'], kw['n_filt'], kw['n_mfcc'])


# ---- the launchers' dispatch, restated (mfcc_general_device.h: general_is_pow2, general_blue_log2; kernels.hip) ------------
def is_pow2(n_fft):
    """lengths that take the packed real transform: powers of two from 64 on"""
    return n_fft & (n_fft - 1) == 0 and n_fft >= 64


def blue_log2(n_fft):
    """log2 of the Bluestein length: the next power of two >= 2 n_fft - 1, at least 128"""
    b = 7
    while (1 << b) < 2 * n_fft - 1:
        b += 1
    return b


def instantiation(n_fft):
    """(form, BITS) of the kernel template the launchers pick for n_fft"""
    if is_pow2(n_fft):
        return 'pow2', (n_fft // 2).bit_length() - 1
    return 'blue', blue_log2(n_fft)


DISPATCHED = [('pow2', b) for b in (5, 6, 7, 8, 9, 10)] + [('blue', b) for b in (7, 8, 9, 10, 11)]      # with_general_bits


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def stream_kinds(n_fft):
    """[(stream number, kind)]: two tones in noise, a few LSBs of noise, silence (the eps clip), and the full-scale square
    wave -- except at n_fft 17, where the square wave (period 2 * 27 samples against a 17-sample frame: whole frames are
    constant, every bin but the first is a difference of equal numbers) is ill-conditioned in float32 for the reference itself
    (2.0 absolute on the CPU)"""
    kinds = [(2, 'tone_noise'), (5, 'tone_noise'), (3, 'quiet'), (4, 'zeros')]
    if n_fft != 17:
        kinds.append((7, 'square'))
    return kinds


def offline_inputs(n_fft, n_samples=N_SAMPLES):
    """[(kind, float64 audio)]"""
    return [(k, synth.stream_pcm(s, n_samples, k).astype(np.float64) / 32768.0) for s, k in stream_kinds(n_fft)]


def frames_of(audio, window, hop):
    """Q1: every full window of ``audio`` -> [n_frames, window]"""
    audio = np.asarray(audio)
    starts = sr.frame_starts(len(audio), window, hop)
    return audio[starts[:, None] + np.arange(window)[None, :]]


# ---- the oracle's pipeline with every array float32 ------------------------------------------------------------------------
def _chirp(n, n_fft):
    """exp(-i pi n^2 / n_fft), the angle from n^2 mod 2 n_fft (exact integers)"""
    r = (np.asarray(n, dtype=np.int64) ** 2) % (2 * n_fft)
    return np.exp(-1j * np.pi * r / n_fft).astype(np.complex64)


def _bluestein_rfft32(x, n_fft):
    """the first n_fft // 2 + 1 bins of the DFT of x [..., n_fft] float32 as a circular convolution with the chirp: complex64
    transforms of length L = 2^blue_log2(n_fft)"""
    L = 1 << blue_log2(n_fft)
    w = _chirp(np.arange(n_fft), n_fft)
    a = np.zeros(x.shape[:-1] + (L,), dtype=np.complex64)
    a[..., :n_fft] = x * w
    b = np.zeros(L, dtype=np.complex64)
    m = np.arange(-(n_fft - 1), n_fft)
    b[m % L] = np.conj(_chirp(m, n_fft))
    A, B = scipy.fft.fft(a), scipy.fft.fft(b)
    assert A.dtype == np.complex64 and B.dtype == np.complex64
    c = scipy.fft.ifft(A * B)
    bins = n_fft // 2 + 1
    return (c[..., :bins] * w[:bins]).astype(np.complex64)


def float32_restatement(frames, n_fft, n_filt, n_mfcc, sample_rate=16000, with_mels=False):
    """frames [n, window] -> MFCCs [n, n_mfcc] float32 (with_mels: and the log-mel energies [n, n_filt] float32): Q2-Q7 of
    oracle/sonopy_restated.py with float32 arrays -- scipy.fft.rfft of float32 frames for the power-of-two lengths the kernels
    transform directly, the Bluestein structure (chirp, scipy.fft.fft / ifft of length L in complex64) for the others"""
    frames = np.asarray(frames)
    x = np.zeros(frames.shape[:-1] + (n_fft,), dtype=np.float32)          # Q2: crop, or zero-pad, to n_fft samples
    n = min(n_fft, frames.shape[-1])
    x[..., :n] = frames[..., :n].astype(np.float32)
    spec = scipy.fft.rfft(x) if is_pow2(n_fft) else _bluestein_rfft32(x, n_fft)
    assert spec.dtype == np.complex64
    powers = (spec.real ** 2 + spec.imag ** 2) / np.float32(n_fft)       # Q3
    filters = sr.filterbanks(sample_rate, n_filt, powers.shape[-1]).astype(np.float32)       # Q4
    eps = np.float32(sr.EPS)
    mels = np.log(np.clip(np.dot(powers, filters.T), eps, None))          # Q5
    mfccs = dct(mels, norm='ortho')[..., :n_mfcc]                         # Q6
    mfccs[..., 0] = np.log(np.clip(np.sum(powers, -1, dtype=np.float32), eps, None))         # Q7
    assert powers.dtype == mels.dtype == mfccs.dtype == np.float32
    return (mfccs, mels) if with_mels else mfccs
