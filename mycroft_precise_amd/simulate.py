"""
False-positive simulation over long recordings: what the reference's ``precise-simulate`` reports per recording and in
total (scripts/simulate.py:106-129), and the not-wake-word buckets of its annoyance estimate
(annoyance_estimator.py:56-73) -- computed for all recordings in one device call (``HipRunner.simulate``).

Reading wav files is left to the caller: every function here takes the recordings as sample arrays.
"""
from dataclasses import dataclass

import numpy as np

from .params import pr


@dataclass
class Metric:
    """The running sums behind one block of the report (simulate.py:45-80)."""
    chunk_size: int
    seconds: float = 0.0
    activated_chunks: int = 0
    activations: int = 0
    activation_sum: float = 0.0

    @property
    def days(self) -> float:
        return self.seconds / 86400.0

    @property
    def chunks(self) -> float:
        """network evaluations the audio amounts to: one per ``chunk_size`` samples"""
        return self.seconds * pr.sample_rate / self.chunk_size

    def add(self, other: 'Metric'):
        self.seconds += other.seconds
        self.activated_chunks += other.activated_chunks
        self.activations += other.activations
        self.activation_sum += other.activation_sum

    def info_string(self, title: str) -> str:
        lines = ['=== %s ===' % title,
                 'Hours: %.2f' % (self.days * 24),
                 'Activations / Day: %.2f' % (self.activations / self.days),
                 'Activated Chunks / Day: %.2f' % (self.activated_chunks / self.days),
                 'Average Activation (*100): %.2f' % (100.0 * self.activation_sum / self.chunks)]
        return '\n'.join(lines)


def default_thresholds() -> np.ndarray:
    """The 1000 thresholds of the annoyance estimate: a sigmoid over linspace(-20, 20) (annoyance_estimator.py:52)."""
    return 1 / (1 + np.exp(-np.linspace(-20, 20, 1000)))


def _recordings(audios):
    """the recordings as arrays, empty ones left out (simulate.py:110 skips them)"""
    return [a for a in (np.asarray(a) for a in audios) if a.size]


def simulate_recordings(runner, audios, chunk_size: int = 4096, threshold: float = 0.5):
    """-> (one Metric per non-empty recording, in order; their total): simulate.py:106-129 without the per-file loop.
    ``runner`` a one-model ``HipRunner``."""
    audios = _recordings(audios)
    rows, _, _ = runner.simulate(audios, chunk_size, threshold)
    total = Metric(chunk_size)
    metrics = []
    for audio, row in zip(audios, rows):
        m = Metric(chunk_size, len(audio) / pr.sample_rate, int(row['activated_chunks']), int(row['activations']),
                   float(row['activation_sum']))
        metrics.append(m)
        total.add(m)
    return metrics, total


def nww_buckets(runner, audios, thresholds=None, chunk_size: int = 4096) -> np.ndarray:
    """``nww_buckets`` of compute_nww_annoyances (annoyance_estimator.py:63-71): per threshold, the windows of all recordings
    whose prediction lies above it.  float64 as the reference accumulates it ([K, n] on a K-model engine)."""
    thresholds = default_thresholds() if thresholds is None else thresholds
    _, buckets, _ = runner.simulate(_recordings(audios), chunk_size, 0.5, thresholds)
    return buckets.astype(np.float64)
