"""
Judging a trained model: what the reference's ``precise-test`` (confusion counts and failing files at a threshold),
``precise-graph`` (false-positive against false-negative rate over a threshold sweep) and ``precise-calc-threshold`` (the
``(mu, std)`` a ``ThresholdDecoder`` is built from) compute from predictions and targets.

Two forms live here:

``Stats(outputs, targets, filenames)``
    the reference's object (stats.py:39-115), on the host, one threshold per call.  The lists of failing files come from
    here: they need the N predictions anyway, and N floats are cheap to bring back.

``Sweep``
    one network's counts for a whole table of thresholds plus the calibration summary, computed next to the predictions on
    the device in one call (``pe_stats_scores`` / ``pe_test_clips`` / ``pe_trainer_stats_models``) -- for
    every network of a K-model engine or a ``TrainerGroup`` at once.  ``sweep_scores``, ``HipRunner.test_clips``,
    ``Trainer.stats`` and ``TrainerGroup.stats`` return sweeps.

    sweeps = group.stats(graph_thresholds(decoder))             # K networks x 98 thresholds, one device call
    x, y = roc_points(sweeps[0])                                # what precise-graph plots
    save_threshold('hey-computer.npz', calc_threshold(sweeps[0]))

There is no CPU fallback for the sweeps: without the HIP library or a GPU they raise.
"""
from math import sqrt

import numpy as np

from .params import inject_params, save_params

_COUNTS = '''=== Counts ===
False Positives: {false_pos}
True Negatives: {true_neg}
False Negatives: {false_neg}
True Positives: {true_pos}'''

_SUMMARY = '''
=== Summary ===
{num_correct} out of {total}
{accuracy_ratio:.2%}

{false_pos_ratio:.2%} false positives
{false_neg_ratio:.2%} false negatives
'''


class Stats:
    """Predictions of one model on one dataset, with the reference's questions about them (stats.py:39-115).

    Every comparison is numpy's, as the reference makes it: a float32 array against a Python float is compared in float32
    (``compare='f32'`` of the device calls).  ``calc_metric`` and the file lists use ``>``, ``num_correct`` uses ``>=``; a
    target is positive when ``astype(bool)`` says so, while ``num_positives`` / ``num_negatives`` count ``> 0.5`` / ``< 0.5``."""

    def __init__(self, outputs, targets, filenames):
        self.outputs = np.array(outputs)
        self.targets = np.array(targets)
        self.filenames = filenames
        self.num_positives = int((self.targets > 0.5).sum())
        self.num_negatives = int((self.targets < 0.5).sum())

    def __len__(self):
        return len(self.outputs)

    # -- one threshold ----------------------------------------------------------------------------------------------
    def _fired(self, threshold):
        return self.outputs > threshold

    def calc_metric(self, is_correct: bool, actual_output: bool, threshold=0.5) -> int:
        """samples the model got right (wrong) while firing (staying silent): ``calc_metric(False, True)`` = false positives"""
        fired = self._fired(threshold)
        right = fired == self.targets.astype(bool)
        return int(((right == is_correct) & (fired == actual_output)).sum())

    def false_positives(self, threshold=0.5):
        return self.calc_metric(False, True, threshold) / max(1, self.num_negatives)

    def false_negatives(self, threshold=0.5):
        return self.calc_metric(False, False, threshold) / max(1, self.num_positives)

    def num_correct(self, threshold=0.5):
        return ((self.outputs >= threshold) == self.targets.astype(bool)).sum()

    def num_incorrect(self, threshold=0.5):
        return len(self) - self.num_correct(threshold)

    def accuracy(self, threshold=0.5):
        return self.num_correct(threshold) / max(1, len(self))

    def to_dict(self, threshold=0.5) -> dict:
        return {name: self.calc_metric(right, fired, threshold)
                for name, right, fired in (('true_pos', True, True), ('true_neg', True, False),
                                           ('false_pos', False, True), ('false_neg', False, False))}

    def counts_str(self, threshold=0.5) -> str:
        return _COUNTS.format(**self.to_dict(threshold))

    def summary_str(self, threshold=0.5) -> str:
        return _SUMMARY.format(num_correct=self.num_correct(threshold), total=len(self), accuracy_ratio=self.accuracy(threshold),
                               false_pos_ratio=self.false_positives(threshold), false_neg_ratio=self.false_negatives(threshold))

    # -- which files ------------------------------------------------------------------------------------------------
    @staticmethod
    def matches_sample(output, target, threshold, is_correct, actual_output) -> bool:
        """is this sample of the class (is_correct, actual_output), e.g. (False, False) a false negative?"""
        fired = bool(output > threshold)
        return (fired == bool(target)) == is_correct and actual_output == fired

    def calc_filenames(self, is_correct: bool, actual_output: bool, threshold=0.5) -> list:
        return [name for output, target, name in zip(self.outputs, self.targets, self.filenames)
                if self.matches_sample(output, target, threshold, is_correct, actual_output)]

    # -- the npz of precise-graph -----------------------------------------------------------------------------------
    def to_np_dict(self) -> dict:
        return {'outputs': self.outputs, 'targets': self.targets, 'filenames': np.array(self.filenames)}

    @staticmethod
    def from_np_dict(data) -> 'Stats':
        return Stats(data['outputs'], data['targets'], data['filenames'])


class Sweep:
    """One network's device result: for ``thresholds[j]`` the arrays ``true_pos[j]``, ``true_neg[j]``, ``false_pos[j]``,
    ``false_neg[j]`` (``Stats.calc_metric``, ``>``) and ``num_correct[j]`` (``Stats.num_correct``, ``>=``), the class counts
    ``n`` / ``n_pos`` / ``n_neg`` / ``n_other`` / ``n_nan`` and the calibration summary ``n_unsaturated`` / ``n_fit`` /
    ``logit_mean`` / ``logit_std``.  ``counts`` keeps the raw device record (``pos_gt``, ``neg_gt``, ``pos_ge``, ``neg_ge``).

    A target in (0, 0.5] belongs to neither class -- the reference's own definitions disagree about it -- so a sweep over
    such targets is refused by name instead of one definition being picked: ValueError naming ``n_other``."""

    def __init__(self, thresholds, counts, summary, compare='f32'):
        self.thresholds = np.array(thresholds, dtype=np.float64).reshape(-1)
        self.counts = np.asarray(counts)
        self.compare = compare
        for name in ('n', 'n_pos', 'n_neg', 'n_other', 'n_nan', 'n_unsaturated', 'n_fit'):
            setattr(self, name, int(summary[name]))
        self.logit_mean, self.logit_std = float(summary['logit_mean']), float(summary['logit_std'])
        if self.n_other:
            raise ValueError('n_other = %d of the %d targets lie in (0, 0.5]: neither positive (> 0.5) nor negative (== 0), and the '
                             "reference's own definitions disagree about them" % (self.n_other, self.n))
        self.true_pos = self.counts['pos_gt'].astype(np.int64)
        self.false_pos = self.counts['neg_gt'].astype(np.int64)
        self.false_neg = self.n_pos - self.true_pos
        self.true_neg = self.n_neg - self.false_pos
        self.num_correct = self.counts['pos_ge'] + (self.n_neg - self.counts['neg_ge'])

    def __len__(self):
        return self.n

    def false_positives(self) -> np.ndarray:
        """``Stats.false_positives`` at every threshold"""
        return self.false_pos / max(1, self.n_neg)

    def false_negatives(self) -> np.ndarray:
        return self.false_neg / max(1, self.n_pos)

    def accuracy(self) -> np.ndarray:
        return self.num_correct / max(1, self.n)

    def to_dict(self, j: int = 0) -> dict:
        """``Stats.to_dict(thresholds[j])``"""
        return {name: int(getattr(self, name)[j]) for name in ('true_pos', 'true_neg', 'false_pos', 'false_neg')}


def sweeps_of(thresholds, counts, summary, compare) -> list:
    """the (counts [rows, T], summary [rows]) pair of a device call -> one ``Sweep`` per row"""
    return [Sweep(thresholds, counts[r], summary[r], compare) for r in range(len(summary))]


def sweep_scores(runner, outputs, targets, thresholds=(0.5,), compare='f32'):
    """Predictions the caller holds -> a ``Sweep`` (``outputs`` [N] or [N, 1]), or a list of them (``outputs`` [K, N] or
    [K, N, 1], up to 16 rows sharing ``targets``).  ``runner``: the ``HipRunner`` whose device does the counting."""
    outputs = np.asarray(outputs, dtype=np.float32)
    targets = np.asarray(targets, dtype=np.float32).reshape(-1)
    many = not (outputs.ndim == 1 or (outputs.ndim == 2 and outputs.shape[1] == 1))         # [N] and [N, 1]: one network
    rows = outputs.reshape(outputs.shape[0], -1) if many else outputs.reshape(1, -1)
    counts, summary = runner.engine.stats_scores(rows, targets, thresholds, compare)
    thr = np.array(thresholds, dtype=np.float64, ndmin=1)
    sweeps = sweeps_of(thr, counts, summary, compare)
    return sweeps if many else sweeps[0]


def graph_thresholds(decoder, resolution: int = 100) -> list:
    """the raw-output thresholds precise-graph sweeps (scripts/graph.py:147-148): the decoder's inverse at ``resolution``
    evenly spaced confidences, the two ends left out"""
    return [decoder.encode(c) for c in np.linspace(0.0, 1.0, resolution)[1:-1]]


def roc_points(sweep):
    """-> (x, y): false-positive and false-negative rate per threshold, the curve precise-graph plots (graph.py:150-151)"""
    return sweep.false_positives(), sweep.false_negatives()


def calc_threshold(result, smoothing: float = 1.2):
    """precise-calc-threshold (scripts/calc_threshold.py:66-77): -> ``(mu, std * smoothing)`` of the logit of the unsaturated
    predictions on positive samples, or None when no prediction is unsaturated (the script's "No data").

    A ``Sweep`` carries both numbers from the device (float64 logarithm and sums).  A ``Stats`` -- e.g. one
    loaded from a ``precise-graph`` npz -- is evaluated on the host with the script's own numpy expression."""
    if isinstance(result, Sweep):
        if result.n_unsaturated == 0:
            return None
        return result.logit_mean, result.logit_std * smoothing
    outputs, targets = np.asarray(result.outputs), np.asarray(result.targets)
    keep = (outputs != 0) & (outputs != 1)
    if keep.sum() == 0:
        return None
    outputs, targets = outputs[keep], targets[keep]
    logits = -np.log(1 / outputs - 1)
    pos = logits[targets > 0.5]
    mu = pos.mean().item()
    return mu, sqrt(np.mean((pos - mu) ** 2)) * smoothing


def save_threshold(model_name: str, mu_std):
    """Make ``(mu, std)`` the model's ``threshold_config`` and write its ``.params``: ``Listener(model_name)`` and the
    runners then decode with the fitted table (calc_threshold.py:80-84)."""
    pr = inject_params(model_name)
    pr.__dict__.update(threshold_config=((float(mu_std[0]), float(mu_std[1])),))
    save_params(model_name)
