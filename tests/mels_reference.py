"""CPU reference for models trained on Vectorizer.mels features (vectorization.py:32-35): a restatement built from what
oracle/ already exports.  TEST INFRASTRUCTURE ONLY.

  * rows: ``sonopy_restated.mel_spec`` -- safe_log(power_spec . filters^T), no DCT, coefficient 0 NOT replaced;
  * sizes: ``oracle.listener.Params(vectorizer=1)``, whose ``feature_size`` is ``n_filt`` (params.py:99-109);
  * ``vectorize_raw`` / ``vectorize`` dispatching on ``pr.vectorizer`` as vectorization.py:46-84 does;
  * the network: ``keras_gru.predict``;
  * ``MelsListener``: ``OracleListener`` with the window ``pr.feature_size`` wide (the INTENT of network_runner.py:104,144, whose
    ``n_mfcc``-wide allocation is what keeps the reference's own Listener from streaming such a model) and ``vectorize_raw``
    dispatching to ``mel_spec``;
  * ``BatchedMels``: the same arithmetic for B lock-step streams (``BatchedOracle``'s bookkeeping).

Pinned by tests/golden/vectorize_mels.npz, which the reference's own ``vectorize`` / ``vectorize_raw`` produced
(tests/test_mels_host.py)."""
import numpy as np

from oracle import keras_gru
from oracle import listener as ol
from oracle import sonopy_restated as sr


def params(**kw):
    kw.setdefault('vectorizer', 1)
    return ol.Params(**kw)


def row_width(pr):
    """values per frame: feature_size without the deltas"""
    return pr.n_filt if pr.vectorizer == 1 else pr.n_mfcc


def vectorize_raw(audio, pr):
    """vectorization.py:46-50 with the dispatch on pr.vectorizer (:31-43)"""
    if len(audio) == 0:
        raise ValueError('Cannot vectorize empty audio!')
    if pr.vectorizer == 1:
        return sr.mel_spec(audio, pr.sample_rate, (pr.window_samples, pr.hop_samples), pr.n_fft, pr.n_filt)
    return ol.vectorize_raw(audio, pr)


def vectorize(audio, pr):
    """vectorization.py:62-84: last max_samples -> rows -> left zero pad / tail crop"""
    if len(audio) > pr.max_samples:
        audio = audio[-pr.max_samples:]
    feats = vectorize_raw(audio, pr)
    if len(feats) < pr.n_features:
        feats = np.concatenate([np.zeros((pr.n_features - len(feats), feats.shape[1])), feats])
    return feats[-pr.n_features:]


def inputs_of(window, pr):
    """[T, W] -> what the network reads: [T, feature_size]"""
    return ol.add_deltas(window) if pr.use_delta else window


def predict(windows, weights, pr):
    """[N, T, W] float64 windows -> raw outputs float32 [N]"""
    windows = np.asarray(windows)
    if pr.use_delta:
        windows = np.stack([ol.add_deltas(w) for w in windows])
    return keras_gru.predict(windows, weights)[:, 0]


def mels_from_frames(frames, pr):
    """frames [..., window] (every full window, sonopy Q1) -> log-mel rows [..., n_filt]: mel_spec from Q2 on"""
    spec = np.fft.rfft(np.asarray(frames, dtype=np.float64), n=pr.n_fft)
    powers = (spec.real ** 2 + spec.imag ** 2) / pr.n_fft
    return sr.safe_log(np.dot(powers, sr.filterbanks(pr.sample_rate, pr.n_filt, powers.shape[-1]).T))


class MelsListener(ol.OracleListener):
    """network_runner.py:98-153 for one stream, the window pr.feature_size wide (without the deltas, which update adds)"""

    def clear(self):
        self.window_audio = np.array([])
        self.mfccs = np.zeros((self.pr.n_features, row_width(self.pr)))

    def update_vectors(self, stream):
        if isinstance(stream, np.ndarray):
            buffer_audio = stream
        else:
            chunk = stream if isinstance(stream, (bytes, bytearray)) else stream.read(self.chunk_size)
            if len(chunk) == 0:
                raise EOFError
            buffer_audio = ol.buffer_to_audio(chunk)
        self.window_audio = np.concatenate((self.window_audio, buffer_audio))
        if len(self.window_audio) >= self.pr.window_samples:
            new = vectorize_raw(self.window_audio, self.pr)
            self.window_audio = self.window_audio[len(new) * self.pr.hop_samples:]
            if len(new) > len(self.mfccs):
                new = new[-len(self.mfccs):]
            self.mfccs = np.concatenate((self.mfccs[len(new):], new))
        return self.mfccs


class BatchedMels:
    """B lock-step streams (equal chunks, cleared together): per stream exactly MelsListener's state and arithmetic"""

    def __init__(self, weights, n_streams, pr):
        self.pr, self.weights, self.n = pr, weights, n_streams
        self.clear()

    def clear(self):
        self.window_audio = np.zeros((self.n, 0))
        self.mfccs = np.zeros((self.n, self.pr.n_features, row_width(self.pr)))

    def update_vectors(self, pcm):
        """int16 [B, chunk] -> windows [B, T, W] float64"""
        pr = self.pr
        audio = pcm.astype(np.float32) / np.float32(32768.0)              # util.py:35-37
        self.window_audio = np.concatenate((self.window_audio, audio.astype(np.float64)), axis=1)
        length = self.window_audio.shape[1]
        if length >= pr.window_samples:
            starts = sr.frame_starts(length, pr.window_samples, pr.hop_samples)
            idx = starts[:, None] + np.arange(pr.window_samples)[None, :]
            new = mels_from_frames(self.window_audio[:, idx], pr)          # [B, n, W]
            n_new = new.shape[1]
            self.window_audio = self.window_audio[:, n_new * pr.hop_samples:]
            if n_new > pr.n_features:
                new = new[:, -pr.n_features:]
            self.mfccs = np.concatenate((self.mfccs[:, new.shape[1]:], new), axis=1)
        return self.mfccs

    def update_raw(self, pcm):
        """-> raw network outputs float32 [B]"""
        return predict(self.update_vectors(pcm), self.weights, self.pr)
