"""
The annoyance estimate of ``precise-train-optimize`` (annoyance_estimator.py:30-112) on bucket arrays.

The reference's estimator models what a network costs its user per day at each of 1000 thresholds: a missed wake word costs
twice as much at every repeated attempt, which for a miss ratio p sums to ``1 / (1 - 2p) - 1`` per interaction (infinite from
p = 0.5 on), and an activation on ambient noise costs a constant.  Both inputs are counts of predictions above each threshold,
and both are counted on the device here:

    ww_buckets   ``pos_gt`` of a ``compare='f64'`` sweep over ``simulate.default_thresholds()`` (``Trainer.stats``,
                 ``TrainerGroup.stats``, ``HipRunner.test_clips``): wake-word samples above each threshold, n_ww of them
    nww_buckets  ``simulate.nww_buckets``: windows of the noise recordings above each threshold, nww_seconds of audio

so that ``estimate`` is left with a handful of float64 operations per threshold, on the host.
"""
from collections import namedtuple

import numpy as np

from .simulate import default_thresholds

AnnoyanceEstimate = namedtuple('AnnoyanceEstimate', 'annoyance ww_annoyance nww_annoyance threshold')


def ww_annoyances(ww_buckets, n_ww, interaction_estimate=100):
    """per threshold the annoyance per day from wake words that were not recognised (annoyance_estimator.py:85-92)"""
    miss = 1 - np.asarray(ww_buckets) / n_ww
    per_interaction = np.divide(1, 1 - 2 * miss, where=miss < 0.5) - 1
    per_interaction[miss >= 0.5] = float('inf')
    return interaction_estimate * per_interaction


def nww_annoyances(nww_buckets, nww_seconds, ambient_annoyance=1.0):
    """per threshold the annoyance per day from activations on ambient noise (annoyance_estimator.py:72-73)"""
    per_hour = np.asarray(nww_buckets, dtype=np.float64) * 60 * 60 / nww_seconds
    return ambient_annoyance * per_hour * 24


def estimate(ww_buckets, n_ww, nww_buckets, nww_seconds, interaction_estimate=100, ambient_annoyance=1.0, thresholds=None):
    """-> ``AnnoyanceEstimate(annoyance, ww_annoyance, nww_annoyance, threshold)`` at the threshold where the sum of both
    annoyances is smallest (the first such threshold), as ``AnnoyanceEstimator.estimate`` returns it.  ``thresholds``: the
    table both bucket arrays were counted over (default: ``simulate.default_thresholds()``)."""
    thresholds = default_thresholds() if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    ww = ww_annoyances(ww_buckets, n_ww, interaction_estimate)
    nww = nww_annoyances(nww_buckets, nww_seconds, ambient_annoyance)
    if not (ww.shape == nww.shape == thresholds.shape):
        raise ValueError('bucket arrays of %r and %r entries for %r thresholds' % (ww.shape, nww.shape, thresholds.shape))
    total = ww + nww
    best = np.argmin(total)
    return AnnoyanceEstimate(annoyance=total[best], ww_annoyance=ww[best], nww_annoyance=nww[best], threshold=thresholds[best])
