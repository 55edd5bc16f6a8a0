#!/usr/bin/env python3
"""
Write tests/golden/stats.npz: what the reference's own ``Stats`` (precise/stats.py), ``ThresholdDecoder.encode``
(precise/threshold_decoder.py), ``AnnoyanceEstimator.compute_ww_annoyances`` / ``estimate`` (precise/annoyance_estimator.py)
and ``CalcThresholdScript.run`` (precise/scripts/calc_threshold.py) compute for two small seeded sets of predictions.

    python tools/make_stats_fixture.py --reference /path/to/mycroft-precise

``precise.stats`` and ``precise.threshold_decoder`` import with numpy alone.  The estimator and the script import packages they
never use on this path (prettyparse, pyache, fitipy, sonopy, speechpy, wavio): those are replaced by empty stub modules.  Only
file access and ``model.predict`` are stood in for, none of the reference's text is edited:

  * ``AnnoyanceEstimator.estimate`` walks ``glob(noise_folder/*.wav)``, loads each file (``_load_inputs``) and asks the model
    for predictions: ``glob`` returns three names, ``_load_inputs`` returns (the name, a length in samples), ``model.predict``
    returns that name's seeded predictions;
  * ``CalcThresholdScript.run`` reads an npz with ``np.load`` (without ``allow_pickle``, which today's numpy refuses for the
    object array the script expects), then ``inject_params`` / ``save_params`` read and write ``<model>.params``: ``np.load``
    hands over the dict the file would hold, the two params functions keep their hands off the disk, and the result is read
    from ``pr.threshold_config``.  The script could be driven this way, so its golden is in the file.

The sets -- ``a``: N = 65, ``b``: N = 2000 -- hold float32 predictions sigmoid(logit) with |logit| <= 20 and a spread of the
positive logits of well over 0.1, a few of them exactly 0.0 and 1.0, and 0 / 1 targets.  One threshold of every sweep equals a
prediction, so ``>`` and ``>=`` differ there.  Per set and threshold: the four ``to_dict`` counts, ``num_correct``,
``num_incorrect``, ``accuracy``, ``false_positives``, ``false_negatives``; at two thresholds ``counts_str``, ``summary_str`` and
the four ``calc_filenames`` lists (as indices); the decoder's graph thresholds; the wake-word annoyances and the estimate; the
script's ``(mu, std)``.
"""
import argparse
import os
import sys
import types

import numpy as np

from reference_stubs import install_stubs

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'stats.npz')

SIZES = {'a': 65, 'b': 2000}
NOISE_WINDOWS = (40, 300, 1)                # predictions per stood-in noise file
NOISE_SAMPLES = (170000, 1234567, 30000)    # ... and its length in samples
INTERACTION_ESTIMATE, AMBIENT_ANNOYANCE = 100, 1.0
SMOOTHING = 1.2


def make_set(rng, n):
    """float32 predictions [n, 1] and 0 / 1 targets [n, 1]: positives around logit +2, negatives around -3, both wide"""
    y = (rng.random(n) < 0.4).astype(np.float32)
    logit = np.where(y > 0.5, rng.normal(2.0, 2.5, n), rng.normal(-3.0, 2.5, n)).clip(-20, 20)
    p = (1 / (1 + np.exp(-logit))).astype(np.float32)
    idx = rng.permutation(n)
    p[idx[:2]] = 0.0
    p[idx[2:4]] = 1.0
    y[idx[0]], y[idx[1]], y[idx[2]], y[idx[3]] = 1.0, 0.0, 1.0, 0.0
    return p.reshape(-1, 1), y.reshape(-1, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', required=True, help='a checkout of the reference implementation')
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()

    stubbed = install_stubs(('prettyparse', 'pyache', 'fitipy', 'sonopy', 'speechpy', 'wavio'))
    sys.path.insert(0, os.path.abspath(args.reference))
    from precise.params import pr
    from precise.stats import Stats
    from precise.threshold_decoder import ThresholdDecoder
    from precise import annoyance_estimator
    from precise.scripts import calc_threshold

    out = {}
    decoder = ThresholdDecoder(pr.threshold_config, pr.threshold_center)
    graph = [decoder.encode(i) for i in np.linspace(0.0, 1.0, 100)[1:-1]]          # scripts/graph.py:148
    out['threshold_config'] = np.array(pr.threshold_config, dtype=np.float64)
    out['threshold_center'] = np.float64(pr.threshold_center)
    out['graph_thresholds'] = np.array(graph, dtype=np.float64)

    rng = np.random.default_rng(20261019)
    noise_pred = {'noise%d.wav' % i: (1 / (1 + np.exp(-rng.normal(-4.0, 3.0, n)))).astype(np.float32).reshape(-1, 1)
                  for i, n in enumerate(NOISE_WINDOWS)}
    noise_len = dict(zip(noise_pred, NOISE_SAMPLES))
    out['noise_predictions'] = np.concatenate([noise_pred[k].reshape(-1) for k in noise_pred])
    out['noise_windows'] = np.array(NOISE_WINDOWS, dtype=np.int64)
    out['noise_samples'] = np.array(NOISE_SAMPLES, dtype=np.int64)
    out['sample_rate'] = np.int64(pr.sample_rate)

    # file access and model.predict of the estimator, stood in for
    annoyance_estimator.glob = lambda pattern: list(noise_pred)
    annoyance_estimator.AnnoyanceEstimator._load_inputs = staticmethod(lambda name, chunk_size=4096: (name, noise_len[name]))
    model = types.SimpleNamespace(predict=lambda inputs, batch_size=None: noise_pred[inputs])

    for key, n in SIZES.items():
        p, y = make_set(rng, n)
        names = ['clip-%04d.wav' % i for i in range(n)]
        stats = Stats(p, y, names)
        # the sweep: 0.5, the graph's thresholds and one that equals a prediction (as the Python float numpy compares with)
        equal = float(p[np.flatnonzero((p.reshape(-1) > 0.2) & (p.reshape(-1) < 0.8))[0], 0])
        thresholds = sorted(set([0.5, equal] + graph))
        assert np.float32(equal) == equal and stats.calc_metric(True, True, equal) + stats.calc_metric(False, True, equal) < \
            int((stats.outputs >= equal).sum())
        out[key + '_outputs'], out[key + '_targets'], out[key + '_filenames'] = p, y, np.array(names)
        out[key + '_thresholds'] = np.array(thresholds, dtype=np.float64)
        out[key + '_equal_threshold'] = np.float64(equal)
        out[key + '_len'] = np.int64(len(stats))
        out[key + '_num_positives'], out[key + '_num_negatives'] = np.int64(stats.num_positives), np.int64(stats.num_negatives)
        dicts = [stats.to_dict(t) for t in thresholds]
        for name in ('true_pos', 'true_neg', 'false_pos', 'false_neg'):
            out[key + '_' + name] = np.array([d[name] for d in dicts], dtype=np.int64)
        out[key + '_num_correct'] = np.array([stats.num_correct(t) for t in thresholds], dtype=np.int64)
        out[key + '_num_incorrect'] = np.array([stats.num_incorrect(t) for t in thresholds], dtype=np.int64)
        out[key + '_accuracy'] = np.array([stats.accuracy(t) for t in thresholds], dtype=np.float64)
        out[key + '_false_positives'] = np.array([stats.false_positives(t) for t in thresholds], dtype=np.float64)
        out[key + '_false_negatives'] = np.array([stats.false_negatives(t) for t in thresholds], dtype=np.float64)
        out[key + '_default_dict'] = np.array([stats.to_dict()[k] for k in ('true_pos', 'true_neg', 'false_pos', 'false_neg')], dtype=np.int64)
        for tag, t in (('half', 0.5), ('equal', equal)):
            out['%s_counts_str_%s' % (key, tag)] = np.array(stats.counts_str(t))
            out['%s_summary_str_%s' % (key, tag)] = np.array(stats.summary_str(t))
            for right in (True, False):
                for fired in (True, False):
                    files = stats.calc_filenames(right, fired, t)
                    out['%s_files_%s_%d%d' % (key, tag, right, fired)] = np.array([names.index(f) for f in files], dtype=np.int64)
                    assert all(Stats.matches_sample(p[names.index(f)], y[names.index(f)], t, right, fired) for f in files)

        # the annoyance estimate (annoyance_estimator.py:75-112)
        est = annoyance_estimator.AnnoyanceEstimator(model, INTERACTION_ESTIMATE, AMBIENT_ANNOYANCE)
        out[key + '_ww_annoyances'] = np.asarray(est.compute_ww_annoyances(p[np.where(y > 0.5)]), dtype=np.float64)
        result = est.estimate(model, p, y, 'noise', 5000)
        out[key + '_estimate'] = np.array([result.annoyance, result.ww_annoyance, result.nww_annoyance, result.threshold], dtype=np.float64)
        out['annoyance_thresholds'] = np.asarray(est.thresholds, dtype=np.float64)

        # precise-calc-threshold (scripts/calc_threshold.py:51-84): np.load and the params file stood in for
        keep = dict(pr.__dict__)
        real_load = np.load
        np.load = lambda name: {'data': np.array({'model': stats.to_np_dict()}, dtype=object)}
        calc_threshold.inject_params = lambda model_name: pr
        calc_threshold.save_params = lambda model_name: None
        try:
            calc_threshold.CalcThresholdScript(types.SimpleNamespace(
                model='model.net', input_file='stats.npz', model_key=None, smoothing=SMOOTHING, center=0.2)).run()
            out[key + '_mu_std'] = np.array(pr.threshold_config[0], dtype=np.float64)
        finally:
            np.load = real_load
            pr.__dict__.clear()
            pr.__dict__.update(keep)
        assert abs(out[key + '_mu_std'][0]) <= 20 and out[key + '_mu_std'][1] / SMOOTHING >= 0.1

    out['smoothing'] = np.float64(SMOOTHING)
    out['interaction_estimate'], out['ambient_annoyance'] = np.float64(INTERACTION_ESTIMATE), np.float64(AMBIENT_ANNOYANCE)
    out['provenance'] = np.array([
        'glue: reference code, unmodified: precise/stats.py (Stats), precise/threshold_decoder.py (ThresholdDecoder.encode), '
        'precise/annoyance_estimator.py (AnnoyanceEstimator.compute_ww_annoyances, estimate; glob, _load_inputs and model.predict '
        'stood in for), precise/scripts/calc_threshold.py (CalcThresholdScript.run; np.load, inject_params and save_params stood '
        'in for); stub modules: ' + ', '.join(stubbed),
        'keras: not used by this fixture',
        'sonopy: not used by this fixture',
        'numpy: ' + np.__version__,
        'python: %d.%d' % sys.version_info[:2],
    ])
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes;', ', '.join('%s: N = %d, mu_std = %r' % (k, SIZES[k], tuple(out[k + '_mu_std'])) for k in SIZES))


if __name__ == '__main__':
    main()
