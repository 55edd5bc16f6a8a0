"""The loop of precise-train-sampled (scripts/train_sampled.py:54-90) restated in numpy over the PUBLIC API of a ``Trainer``:
``predict`` from host memory, the failed and remaining sets by hash, a pluggable order in front of the script's ``islice``,
the metrics line, and ``fit`` on host copies of the selected rows.  ``test_sampled.py`` runs it on a second trainer with the
same seed and initial weights and asks ``SampledTrainer`` for the same selection, lines, file and weights.

Held in turn to the script itself: tests/golden/train_sampled.npz is what the reference's own ``TrainScript.load_sample_data``,
``TrainSampledScript.choose_new_samples`` and ``write_sampling_metrics`` gave in two cycles taken by hand
(tools/make_script_fixtures.py); test_sampled_host.py asks for the same hash table (the LAST duplicate wins; the first does NOT
reproduce it), remaining failed rows, counts and metrics lines."""
import hashlib
from itertools import islice

import numpy as np


def calc_sample_hash(inp, outp) -> str:
    md5 = hashlib.md5()
    md5.update(inp.tobytes())
    md5.update(outp.tobytes())
    return md5.hexdigest()


def errors(predicted, outputs) -> np.ndarray:
    """the key of order 'error': float32 |p - y|, NaN as +infinity"""
    e = np.abs(np.asarray(predicted).reshape(-1).astype(np.float32) - np.asarray(outputs).reshape(-1).astype(np.float32))
    return np.where(np.isnan(e), np.float32(np.inf), e)


def choose_index(remaining, hash_to_ind, predicted, outputs):
    return sorted(remaining, key=hash_to_ind.get)


def choose_error(remaining, hash_to_ind, predicted, outputs):
    hashes = list(remaining)
    index = np.array([hash_to_ind[h] for h in hashes], dtype=np.int64)
    e = errors(predicted, outputs)[index]
    return [hashes[i] for i in np.lexsort((index, -e))]


CHOOSERS = {'index': choose_index, 'error': choose_error}


def lexsort_rows(candidates, predicted, outputs, order):
    """candidate rows in the order `order` takes them"""
    candidates = np.asarray(candidates, dtype=np.int64)
    if order == 'index':
        return np.sort(candidates)
    return candidates[np.lexsort((candidates, -errors(predicted, outputs)[candidates]))]


def run(trainer, inputs, outputs, cycles, epochs, batch_size, num_sample_chunk, order):
    """-> (selected rows after every cycle, the metrics lines, the final set of hashes)"""
    train = (inputs, outputs)
    hash_to_ind = {calc_sample_hash(inp, outp): ind for ind, (inp, outp) in enumerate(zip(*train))}
    samples, selected = set(), []
    metrics, per_cycle = [], []
    for _ in range(cycles):
        predicted = trainer.predict(train[0])
        failed_samples = {
            calc_sample_hash(inp, target)
            for i, (inp, pred, target) in enumerate(zip(train[0], predicted, train[1]))
            if (pred > 0.5) != (target > 0.5)
        }
        remaining_failed_samples = failed_samples - samples
        new = list(islice(CHOOSERS[order](remaining_failed_samples, hash_to_ind, predicted, train[1]), num_sample_chunk))
        samples.update(new)
        selected += [hash_to_ind[h] for h in new]
        correct = float(np.sum((predicted > 0.5) == (train[1] > 0.5)) / len(train[1]))
        metrics.append('{}\t{}'.format(len(samples) / len(train[1]), correct))
        per_cycle.append(list(selected))
        if selected:
            trainer.fit(train[0][selected], train[1][selected], batch_size=batch_size, epochs=epochs)
    return per_cycle, metrics, samples
