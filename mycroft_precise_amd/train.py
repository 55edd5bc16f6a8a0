"""
Training: the ``precise-train`` step of the reference on the GPU.

The reference trains with ``model.fit(train_inputs, train_outputs, batch_size, epochs)`` on ``Sequential([GRU(units,
activation='linear', dropout=0.2), Dense(1, 'sigmoid')])`` compiled with ``rmsprop`` and ``weighted_log_loss``
(scripts/train.py:159-166, model.py:76-90, functions.py:39-50).  ``Trainer`` is that step: forward with Keras' per-gate input
dropout, the weighted log loss, the backward pass and RMSprop all run in HIP kernels (csrc/gru_train_device.h, contract in
DESIGN.md 4.9); this module only shuffles indices and keeps the history.

    trainer = Trainer(params=ModelParams(recurrent_units=20))
    history = trainer.fit(inputs, outputs, batch_size=5000, epochs=10, validation_data=(val_in, val_out))
    trainer.save('hey-computer.npz')            # then HipRunner('hey-computer.npz') / Listener serve it

``GeneratedTrainer`` is the ``fit_generator`` loop of ``precise-train-generated`` over a ``generated.Generator``; ``IncrementalTrainer``
the policy of ``precise-train-incremental`` over a ``mining.Miner``; ``SampledTrainer`` the loop of ``precise-train-sampled``
(the failing samples are chosen on the device) and the samples file of ``precise-train -sf [-is]``.

``TrainerGroup`` trains several candidate networks -- other widths, dropout rates, ``loss_bias`` values, seeds -- on the same
data at once: one resident dataset, one launch per batch for all of them, and each candidate ends with exactly the bits that a
``Trainer`` of its own would have given it.

    group = TrainerGroup([ModelParams(recurrent_units=u, loss_bias=b) for u in (12, 20, 32) for b in (0.5, 0.7)])
    histories = group.fit(inputs, outputs, validation_data=(val_in, val_out))
    group.save(group.best('val_loss'), 'hey-computer.npz')

There is no CPU fallback: without the HIP library or a GPU the constructor raises.
"""
from math import exp

import numpy as np

from ._lib import HipTrainer, dropout_masks            # noqa: F401  (dropout_masks: the kernel's mask function on the host)
from .model import ModelParams, create_model, save_weights
from .params import pr, save_params

# keras.optimizers.RMSprop defaults of Keras 2.2.4 (what compile('rmsprop') builds)
RMSPROP_LR, RMSPROP_RHO, RMSPROP_EPS = 1e-3, 0.9, 1e-7


def flatten_weights(weights: dict) -> np.ndarray:
    """weights dict (one or two GRU layers) -> the trainer's flat float32 vector: per layer kernel | recurrent_kernel | bias,
    then dense_kernel | dense_bias."""
    if len(weights['gru']) not in (1, 2):
        raise ValueError('flatten_weights: %d GRU layers (1..2)' % len(weights['gru']))
    parts = [a for layer in weights['gru'] for a in layer] + [weights['dense_kernel'], weights['dense_bias']]
    return np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in parts])


def _layer_units(units) -> tuple:
    """``recurrent_units`` as a tuple of one or two widths"""
    widths = tuple(int(u) for u in units) if isinstance(units, (tuple, list)) else (int(units),)
    if len(widths) not in (1, 2):
        raise ValueError('units must name one or two GRU layers, got %r' % (units,))
    return widths


def unflatten_weights(flat, feature_size: int, units) -> dict:
    """``units``: an int (one GRU layer) or a tuple of one or two widths"""
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    widths = _layer_units(units)
    shapes, n_in = [], int(feature_size)
    for H in widths:
        shapes += [(n_in, 3 * H), (H, 3 * H), (3 * H,)]
        n_in = H
    shapes += [(n_in, 1), (1,)]
    sizes = [int(np.prod(shape)) for shape in shapes]
    if flat.size != sum(sizes):
        raise ValueError('expected %d values for F = %d, H = %s, got %d' %
                         (sum(sizes), int(feature_size), widths[0] if len(widths) == 1 else widths, flat.size))
    arrays = [a.reshape(shape).copy() for a, shape in zip(np.split(flat, np.cumsum(sizes)[:-1]), shapes)]
    return {'gru': [tuple(arrays[3 * i:3 * i + 3]) for i in range(len(widths))], 'dense_kernel': arrays[-2], 'dense_bias': arrays[-1]}


def _units_of(weights: dict):
    """int for a one-layer network, (H1, H2) for a stacked one; anything else has no training kernel"""
    if len(weights['gru']) not in (1, 2):
        raise NotImplementedError('training: n_layers = %d (1..2)' % len(weights['gru']))
    widths = tuple(int(np.shape(rk)[0]) for _, rk, _ in weights['gru'])
    return widths[0] if len(widths) == 1 else widths


def _frozen_mask(freeze_till, units) -> int:
    """model.py:84-85, layers[:freeze_till]: one bit per layer of the Sequential, two for a one-layer network, three for a
    stacked one"""
    return ((1 << max(0, int(freeze_till))) - 1) & (7 if isinstance(units, tuple) else 3)


class Trainer:
    """``weights``: a weights dict to continue from; None = ``create_model``'s random network for the current ``pr`` and
    ``params.recurrent_units``.  ``params`` supplies ``dropout``, ``loss_bias`` (the reference passes ``1.0 - sensitivity``,
    scripts/train.py:86) and ``freeze_till``.  ``seed`` drives the initial network, the shuffle and the dropout masks.
    ``recurrent_units`` 1..256: up to 32 units ``pe_trainer_create``, wider networks ``pe_trainer_create_wide``
    (the matrix-core kernels of DESIGN.md 4.15); the trainer is the same object either way.  Two-layer ``weights``, or
    ``recurrent_units=(H1, H2)``, train the stacked network GRU(H1, return_sequences) -> GRU(H2) -> Dense
    (``pe_trainer_create_stacked``): ``units`` is then the tuple and ``frozen_mask`` has three bits."""

    def __init__(self, weights=None, params: ModelParams = None, seed: int = 42, device: int = 0, n_features: int = None):
        self.params = params or ModelParams()
        self.seed = int(seed)
        if weights is None:
            weights = create_model(None, self.params, seed=self.seed)
        self.units = _units_of(weights)
        self.feature_size = int(np.shape(weights['gru'][0][0])[0])
        self.n_features = int(pr.n_features if n_features is None else n_features)
        if isinstance(self.units, tuple):
            self._t = HipTrainer(weights, self.n_features, self.feature_size, device=device, stacked=True)
        else:
            self._t = HipTrainer(weights, self.n_features, self.feature_size, device=device, wide=self.units > 32)
        self._rng = np.random.default_rng(self.seed)
        self._step = 0                   # optimizer steps taken so far: the dropout masks' step counter
        self.frozen_mask = _frozen_mask(self.params.freeze_till, self.units)

    # -- the network --------------------------------------------------------------------------------------------------
    @property
    def weights(self) -> dict:
        return unflatten_weights(self._t.get_weights(), self.feature_size, self.units)

    @weights.setter
    def weights(self, weights: dict):
        self._t.set_weights(flatten_weights(weights))

    def save(self, model_name: str):
        """``save_weights`` + ``save_params``: ``HipRunner(model_name)`` / ``Listener`` then serve the trained network."""
        save_weights(model_name, self.weights)
        save_params(model_name)

    # -- evaluation -----------------------------------------------------------------------------------------------------
    def predict(self, inputs) -> np.ndarray:
        """[N, n_features, feature_size] -> raw network outputs float32 [N, 1] (dropout off)."""
        return self._t.evaluate(inputs)[2].reshape(-1, 1)

    def evaluate(self, inputs, outputs):
        """-> (loss, acc): weighted_log_loss with ``params.loss_bias`` and Keras' binary accuracy, dropout off."""
        loss, acc, _ = self._t.evaluate(inputs, outputs, loss_bias=self.params.loss_bias)
        return loss, acc

    def loss_and_grads(self, inputs, outputs, masks=None):
        """-> (loss, gradients as a weights dict, probabilities [N, 1]) of one batch; ``masks`` float32
        [3, N, feature_size] per-gate input dropout masks or None (a stacked network: the pair of layer 0's and layer 1's
        [3, N, H1]).  Changes no state."""
        loss, grads, probs = self._t.loss_grad(inputs, outputs, masks=masks, loss_bias=self.params.loss_bias)
        return loss, unflatten_weights(grads, self.feature_size, self.units), probs.reshape(-1, 1)

    # -- model.fit ------------------------------------------------------------------------------------------------------
    def fit(self, inputs, outputs, batch_size=5000, epochs=10, validation_data=None, shuffle=True, callback=None) -> dict:
        """Keras ``model.fit``: per epoch the (shuffled) samples in batches of ``batch_size``, the last one short; the epoch
        loss is the mean of the batch losses.  ``acc`` is measured after the epoch with dropout off.  ``callback(epoch,
        logs)`` runs after every epoch.  -> history dict of lists ``loss``, ``acc`` (and ``val_loss``, ``val_acc``)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.float32)
        n = inputs.shape[0]
        if n == 0 or int(batch_size) < 1:
            raise ValueError('fit needs at least one sample and batch_size >= 1')
        self._t.set_data(inputs, outputs)
        return self._fit(n, batch_size, epochs, shuffle, callback, lambda: self.evaluate(inputs, outputs),
                         None if validation_data is None else lambda: self.evaluate(*validation_data))

    def _fit(self, n, batch_size, epochs, shuffle, callback, measure, measure_validation, rows=None) -> dict:
        """the epochs of ``fit`` over the resident training set of ``n`` samples (``rows``: over these ``n`` rows of it);
        ``measure()`` -> (loss, acc) after an epoch"""
        p = self.params
        history = {'loss': [], 'acc': []}
        if measure_validation is not None:
            history.update(val_loss=[], val_acc=[])
        for epoch in range(int(epochs)):
            order = self._rng.permutation(n) if shuffle else np.arange(n)
            if rows is not None:
                order = rows[order]
            losses = []
            for a in range(0, n, int(batch_size)):
                losses.append(self._t.step(order[a:a + int(batch_size)], dropout_rate=p.dropout, seed=self.seed, step=self._step,
                                           loss_bias=p.loss_bias, lr=RMSPROP_LR, rho=RMSPROP_RHO, eps=RMSPROP_EPS,
                                           frozen_mask=self.frozen_mask))
                self._step += 1
            logs = {'loss': float(np.mean(losses)), 'acc': measure()[1]}
            if measure_validation is not None:
                logs['val_loss'], logs['val_acc'] = measure_validation()
            for k, v in logs.items():
                history[k].append(v)
            if callback is not None:
                callback(epoch, logs)
        return history

    # -- a training set that stays on the device and grows (scripts/train_incremental.py:96-111) ----------------------
    def set_data(self, inputs, outputs, validation=False):
        """Upload the training (``validation``: the validation) set once; ``append`` / ``Miner.append_to`` add to it and
        ``fit_resident`` trains on it."""
        (self._t.set_validation if validation else self._t.set_data)(inputs, outputs)

    def append(self, inputs, outputs, validation=False):
        """More samples behind the resident training (validation) set; what is there stays (``TrainData.merge``,
        train_incremental.py:101-102, without a new upload)."""
        self._t.append(inputs, outputs, validation=validation)

    def n_samples(self, validation=False) -> int:
        return self._t.n_samples(validation)

    def _evaluate_resident(self, source):
        loss, acc, _ = self._t.evaluate_models(loss_bias=self.params.loss_bias, source=source, want_probs=False)
        return float(loss[0]), float(acc[0])

    def stats(self, thresholds=(0.5,), validation=True, compare='f32'):
        """The network over the resident validation (training) set and, next to the predictions on the device, its confusion
        counts at every threshold plus the calibration summary: -> a ``stats.Sweep``.  Targets in (0, 0.5] are refused by
        name (ValueError naming ``n_other``)."""
        from .stats import sweeps_of
        counts, summary, _ = self._t.stats_models(thresholds=thresholds, compare=compare, source='validation' if validation else 'data')
        return sweeps_of(np.array(thresholds, dtype=np.float64, ndmin=1), counts, summary, compare)[0]

    def fit_resident(self, batch_size=5000, epochs=1, shuffle=True, callback=None, subset=None) -> dict:
        """``fit`` on the resident training set, without an upload: the same steps -- the same weights, bit for bit, as ``fit``
        on the same samples from the same state -- with ``acc`` (and ``val_loss`` / ``val_acc`` when a validation set is
        resident) measured on the resident sets.  The optimizer state carries over from call to call, as it does when the
        reference calls ``model.fit`` again on the model it keeps (train_incremental.py:106-109).

        ``subset``: row indices of the resident set (repeats allowed, order kept): the epochs run over ``subset[perm]`` and
        ``acc`` is measured over exactly those rows -- weights, accumulators and history of ``fit(inputs[subset],
        outputs[subset], ...)`` from the same state, bit for bit."""
        n = self._t.n_samples()
        if n == 0 or int(batch_size) < 1:
            raise ValueError('fit_resident needs a resident training set (set_data / append) and batch_size >= 1')
        validation = (lambda: self._evaluate_resident('validation')) if self._t.n_samples(True) else None
        if subset is None:
            return self._fit(n, batch_size, epochs, shuffle, callback, lambda: self._evaluate_resident('data'), validation)
        rows = np.array(subset, dtype=np.int64).reshape(-1)
        if rows.size == 0 or rows.min() < 0 or rows.max() >= n:
            raise ValueError('subset needs at least one row, each within the resident set of %d samples' % n)

        def measure():
            loss, acc, _ = self._t.evaluate_indices(rows, loss_bias=self.params.loss_bias, want_probs=False)
            return float(loss[0]), float(acc[0])
        return self._fit(rows.size, batch_size, epochs, shuffle, callback, measure, validation, rows=rows)

    def close(self):
        self._t.close()


class TrainerGroup:
    """K candidate networks trained together on ONE resident dataset (``pe_trainer_create_models``; with a
    candidate of more than 32 units ``pe_trainer_create_wide``, DESIGN.md 4.15: widths 1..256 in any mix, the narrow ones with
    the bits they have in a narrow group).

    ``candidates``: a list of ``ModelParams``; ``recurrent_units``, ``dropout``, ``loss_bias`` and ``freeze_till`` mean what
    they mean to ``Trainer``.  One- and two-layer candidates mix (``pe_trainer_create_stacked``): a stacked
    candidate's ``units`` entry is the tuple (H1, H2) and its frozen mask has three bits.  ``seeds[m]`` (default: ``seed`` for every candidate) drives candidate m's initial network and its
    dropout masks; ``weights[m]`` (a weights dict or None) continues candidate m from a given network.  The group shuffles
    ONCE per epoch for all candidates, with the generator ``Trainer(seed=seed)`` uses.  Candidate m gets, bit for bit, what
    ``Trainer(weights[m], candidates[m], seed=seeds[m])`` gets from the same batches."""

    def __init__(self, candidates, seeds=None, weights=None, seed: int = 42, device: int = 0, n_features: int = None):
        self.candidates = list(candidates)
        K = len(self.candidates)
        if K < 1:
            raise ValueError('TrainerGroup needs at least one candidate')
        self.seed = int(seed)
        self.seeds = [self.seed] * K if seeds is None else [int(v) for v in seeds]
        if len(self.seeds) != K:
            raise ValueError('%d seeds for %d candidates' % (len(self.seeds), K))
        weights = [None] * K if weights is None else list(weights)
        if len(weights) != K:
            raise ValueError('%d weights for %d candidates' % (len(weights), K))
        weights = [create_model(None, p, seed=s) if w is None else w for w, p, s in zip(weights, self.candidates, self.seeds)]
        self.units = [_units_of(w) for w in weights]
        sizes = {int(np.shape(w['gru'][0][0])[0]) for w in weights}
        if len(sizes) != 1:
            raise ValueError('the candidates of a group share feature_size, got %s' % sorted(sizes))
        self.feature_size = sizes.pop()
        self.n_features = int(pr.n_features if n_features is None else n_features)
        if any(isinstance(u, tuple) for u in self.units):
            self._t = HipTrainer(weights, self.n_features, self.feature_size, device=device, stacked=True)
        else:
            self._t = HipTrainer(weights, self.n_features, self.feature_size, device=device, wide=max(self.units) > 32)
        self._rng = np.random.default_rng(self.seed)
        self._step = 0
        self.frozen_masks = [_frozen_mask(p.freeze_till, u) for p, u in zip(self.candidates, self.units)]

    def __len__(self):
        return len(self.candidates)

    def _biases(self):
        return [p.loss_bias for p in self.candidates]

    # -- the networks -------------------------------------------------------------------------------------------------
    @property
    def weights(self) -> list:
        return [unflatten_weights(flat, self.feature_size, units)
                for flat, units in zip(self._t.split(self._t.get_weights()), self.units)]

    def save(self, m: int, model_name: str):
        """candidate m as ``Trainer.save`` writes it"""
        save_weights(model_name, self.weights[m])
        save_params(model_name)

    # -- evaluation -----------------------------------------------------------------------------------------------------
    def predict(self, inputs) -> np.ndarray:
        """[N, n_features, feature_size] -> raw network outputs float32 [K, N, 1] (dropout off)"""
        return self._t.evaluate_models(inputs)[2][:, :, None]

    def evaluate(self, inputs, outputs) -> list:
        """-> K pairs (loss, acc), each candidate with its own ``loss_bias``"""
        loss, acc, _ = self._t.evaluate_models(inputs, outputs, loss_bias=self._biases())
        return [(float(a), float(b)) for a, b in zip(loss, acc)]

    def _evaluate_resident(self, source):
        loss, acc, _ = self._t.evaluate_models(loss_bias=self._biases(), source=source, want_probs=False)
        return [float(v) for v in loss], [float(v) for v in acc]

    # -- model.fit ------------------------------------------------------------------------------------------------------
    def fit(self, inputs, outputs, batch_size=5000, epochs=10, validation_data=None, shuffle=True, callback=None) -> list:
        """``Trainer.fit`` for every candidate on the same batches: one upload of the training set, one of the validation
        set, one step call per batch; ``acc`` / ``val_loss`` / ``val_acc`` are measured on the resident sets.
        ``callback(epoch, logs_list)`` runs once per epoch.  -> K history dicts with ``Trainer.fit``'s keys."""
        inputs = np.ascontiguousarray(inputs, dtype=np.float32)
        n, K = inputs.shape[0], len(self)
        if n == 0 or int(batch_size) < 1:
            raise ValueError('fit needs at least one sample and batch_size >= 1')
        self._t.set_data(inputs, outputs)
        if validation_data is not None:
            self._t.set_validation(*validation_data)
        histories = [{'loss': [], 'acc': []} for _ in range(K)]
        if validation_data is not None:
            for h in histories:
                h.update(val_loss=[], val_acc=[])
        rates = [p.dropout for p in self.candidates]
        for epoch in range(int(epochs)):
            order = self._rng.permutation(n) if shuffle else np.arange(n)
            losses = []
            for a in range(0, n, int(batch_size)):
                losses.append(self._t.step_models(order[a:a + int(batch_size)], step=self._step, dropout_rate=rates, seed=self.seeds,
                                                  loss_bias=self._biases(), lr=RMSPROP_LR, rho=RMSPROP_RHO, eps=RMSPROP_EPS,
                                                  frozen_mask=self.frozen_masks))
                self._step += 1
            acc = self._evaluate_resident('data')[1]
            logs_list = [{'loss': float(np.mean([float(batch[m]) for batch in losses])), 'acc': acc[m]} for m in range(K)]
            if validation_data is not None:
                val_loss, val_acc = self._evaluate_resident('validation')
                for m, logs in enumerate(logs_list):
                    logs['val_loss'], logs['val_acc'] = val_loss[m], val_acc[m]
            for h, logs in zip(histories, logs_list):
                for k, v in logs.items():
                    h[k].append(v)
            if callback is not None:
                callback(epoch, logs_list)
        self.histories = histories
        return histories

    def stats(self, thresholds=(0.5,), validation=True, compare='f32') -> list:
        """``Trainer.stats`` for every candidate in one device call: -> K sweeps over the same thresholds"""
        from .stats import sweeps_of
        counts, summary, _ = self._t.stats_models(thresholds=thresholds, compare=compare, source='validation' if validation else 'data')
        return sweeps_of(np.array(thresholds, dtype=np.float64, ndmin=1), counts, summary, compare)

    def best(self, key: str = 'val_loss') -> int:
        """the candidate whose last-epoch ``key`` is smallest (largest for the accuracies); ``'cost'``: the candidate whose
        trial report (``trial_reports``) has the smallest cost"""
        if key == 'cost':
            if not getattr(self, 'reports', None):
                raise ValueError("no 'cost' for this group yet (call trial_reports first)")
            return int(np.argmin([r['cost'] for r in self.reports]))
        if not getattr(self, 'histories', None) or key not in self.histories[0] or not self.histories[0][key]:
            raise ValueError('no %r in the histories of this group (call fit first)' % key)
        last = [h[key][-1] for h in self.histories]
        return int(np.argmax(last) if key.endswith('acc') else np.argmin(last))

    def close(self):
        self._t.close()


def params_cost(n_params: int) -> float:
    """what a network's size costs (train_optimize.py:64-77): flat up to about 11000 parameters, exponential beyond"""
    return 1.0 + exp((n_params - 11000) / 10000)


def trial_reports(group, runner, noise_audios, interaction_estimate=100, ambient_annoyance=1.0, chunk_size: int = 4096) -> list:
    """What a trial of ``precise-train-optimize`` remembers (scripts/train_optimize.py:98-127), for every candidate of a
    ``TrainerGroup`` at once: -> K dicts ``test_stats`` (the confusion counts at 0.5), ``best_threshold``, ``cost`` and
    ``cost_info`` (``params_cost``, ``annoyance``, ``ww_annoyance``, ``nww_annoyance``).

    The wake-word side is counted on the group's resident validation set (``TrainerGroup.stats``, two device calls for all
    candidates); the noise side on ``runner``, a K-model ``HipRunner`` that holds ``group.weights``, over ``noise_audios``
    (``simulate.nww_buckets``, one call).  A group of several widths takes a list of runners, one per width in the order the
    widths first appear in ``group.units``, each a multi-model ``HipRunner`` over that width's weights in group order (a
    multi-model engine holds networks of one width).  The reports are kept as ``group.reports`` for ``group.best('cost')``."""
    from . import annoyance, simulate
    K = len(group)
    thresholds = simulate.default_thresholds()
    recordings = [np.asarray(a) for a in noise_audios]
    if isinstance(runner, (list, tuple)):
        widths = list(dict.fromkeys(group.units))
        if len(runner) != len(widths):
            raise ValueError('trial_reports: %d runners for the %d widths of the group, units = %r' % (len(runner), len(widths), group.units))
        nww = np.zeros((K, len(thresholds)), dtype=np.float64)
        for r, width in zip(runner, widths):
            members = [m for m, u in enumerate(group.units) if u == width]
            engine = r.engine
            last = width[-1] if isinstance(width, tuple) else width          # (an engine's ``units`` is its last GRU layer's)
            if not getattr(engine, '_multi', False) or engine.n_models != len(members) or engine.units != last:
                raise ValueError('trial_reports: the runner of the %d candidate%s of %d units must be a multi-model HipRunner holding '
                                 'their weights in group order' % (len(members), '' if len(members) == 1 else 's', width))
            nww[members] = simulate.nww_buckets(r, recordings, thresholds, chunk_size).reshape(len(members), -1)
    else:
        engine = runner.engine
        multi = getattr(engine, '_multi', False)
        if multi and len(set(group.units)) != 1:
            raise ValueError('trial_reports: a multi-model engine holds networks of one width, the group has units = %r; pass one '
                             'runner per width' % (group.units,))
        if not multi or engine.n_models != K:
            raise ValueError('trial_reports needs a multi-model HipRunner holding the %d networks of the group (HipRunner(weights=group.weights)), '
                             'got one of %d model%s' % (K, engine.n_models, '' if multi else ' (single-model form)'))
        nww = simulate.nww_buckets(runner, recordings, thresholds, chunk_size).reshape(K, -1)
    at_half = group.stats((0.5,), validation=True, compare='f32')
    ww = group.stats(thresholds, validation=True, compare='f64')
    seconds = 0.0
    for a in recordings:                          # (annoyance_estimator.py:67 adds file by file; an empty file adds 0)
        seconds += len(a) / pr.sample_rate
    reports = []
    for m in range(K):
        est = annoyance.estimate(ww[m].counts['pos_gt'], ww[m].n_pos, nww[m], seconds, interaction_estimate, ambient_annoyance, thresholds)
        size = params_cost(int(group._t.n_params[m]))
        reports.append({'test_stats': at_half[m].to_dict(0), 'best_threshold': est.threshold, 'cost': est.annoyance + size,
                        'cost_info': {'params_cost': size, 'annoyance': est.annoyance, 'ww_annoyance': est.ww_annoyance,
                                      'nww_annoyance': est.nww_annoyance}})
    group.reports = reports
    return reports


class IncrementalTrainer:
    """The policy of ``precise-train-incremental`` (scripts/train_incremental.py:113-137) over a ``mining.Miner``.

    Per recording the script draws ``save_test = random() > 0.8``; every chunk whose prediction exceeds ``threshold`` is saved
    -- into the validation folder for a test recording -- and counted; after every chunk, ``not save_test and count >=
    delay_samples and epochs > 0`` retrains for ``epochs`` epochs and resets the count, and the next chunk is judged by the
    retrained model.  Hits of test recordings count but never trigger.  Here the chunks of all recordings are scored in one
    scan; the host walks the ordered hits to the first chunk at which the script would retrain (the cut), appends the hits up
    to it to the trainer's resident sets, runs ``fit_resident``, hands ``trainer.weights`` to the runner and scans again from
    the chunk after the cut.

        trainer.set_data(train_inputs, train_outputs)               # what retrain() loads from the data folder
        inc = IncrementalTrainer(trainer, runner, delay_samples=10, epochs=1)
        hits, retrains = inc.run(audios)

    ``run`` -> (``[(recording, chunk, went_to_test), ...]`` in the order the script saves them, ``[(recording, chunk), ...]``
    the chunks after which it retrained).  ``test_flags``: one bool per recording; None draws them as the script does, from
    ``rng`` (``numpy.random.Generator``; default: a fresh one).  wav files stay with the caller."""

    def __init__(self, trainer, runner, delay_samples: int = 10, epochs: int = 1, batch_size: int = 5000, threshold: float = 0.5,
                 chunk_size: int = 2048, capacity: int = 4096, shuffle: bool = True, miner_cls=None):
        self.trainer, self.runner = trainer, runner
        self.delay_samples, self.epochs, self.batch_size = int(delay_samples), int(epochs), int(batch_size)
        self.threshold, self.chunk_size, self.capacity, self.shuffle = float(threshold), int(chunk_size), max(1, int(capacity)), shuffle
        self.miner_cls = miner_cls
        self.samples_since_train = 0

    def _make_miner(self, audios):
        if self.miner_cls is not None:
            return self.miner_cls(self.runner, audios, chunk_size=self.chunk_size, carry_audio=True)
        from .mining import Miner
        return Miner(self.runner, audios, chunk_size=self.chunk_size, carry_audio=True)

    def run(self, audios, test_flags=None, rng=None):
        audios = list(audios)
        if test_flags is None:
            rng = np.random.default_rng() if rng is None else rng
            test_flags = [bool(rng.random() > 0.8) for _ in audios]                 # train_incremental.py:115
        test_flags = [bool(f) for f in test_flags]
        if len(test_flags) != len(audios):
            raise ValueError('%d test flags for %d recordings' % (len(test_flags), len(audios)))
        miner = self._make_miner(audios)
        offsets = np.asarray(miner.chunk_offsets, dtype=np.int64)
        total = int(offsets[-1])
        flags = np.asarray(test_flags, dtype=bool)
        saved, retrains = [], []
        pos = 0
        try:
            while pos < total:
                hits, n_above, _ = miner.scan(first=pos, threshold=self.threshold, capacity=self.capacity)
                hits = np.asarray(hits, dtype=np.int64)
                rec, chunk = miner.locate(hits)
                # the cut: the first hit in a training recording at which the count reaches delay_samples.  A count that a test
                # recording pushed past it fires at the FIRST chunk of the next training recording, hit or not (:134).
                cut = self._cut(pos, hits, rec, offsets, flags, total, complete=len(hits) == n_above)
                upto = total if cut is None else cut + 1
                take = hits[hits < upto]
                r_take, c_take = rec[:take.size], chunk[:take.size]
                for validation in (False, True):
                    part = take[flags[r_take] == validation]
                    if part.size:
                        miner.append_to(self.trainer, part, validation=validation)
                saved += [(int(r), int(c), bool(flags[r])) for r, c in zip(r_take, c_take)]
                if cut is None and len(hits) < n_above:
                    # capacity ran out before a cut: the count so far stands, go on behind the last hit taken
                    self.samples_since_train += int(take.size)
                    pos = int(take[-1]) + 1
                    continue
                if cut is None:
                    self.samples_since_train += int(take.size)
                    break
                self.samples_since_train = 0
                r_cut = int(np.searchsorted(offsets, cut, side='right') - 1)
                retrains.append((r_cut, int(cut - offsets[r_cut])))
                self.trainer.fit_resident(self.batch_size, self.epochs, shuffle=self.shuffle)
                self.runner.set_weights(self.trainer.weights)
                pos = cut + 1
        finally:
            miner.close()
        return saved, retrains

    def _cut(self, pos, hits, rec, offsets, flags, total, complete):
        """global id of the first chunk >= pos after which the script retrains, given the hits from pos on (all of them when
        ``complete``, else a prefix: then nothing behind the last one is known) -- or None if there is none in what is known"""
        if self.epochs <= 0:
            return None
        horizon = total if complete else (int(hits[-1]) + 1 if len(hits) else pos)
        count = self.samples_since_train
        i = 0
        g = pos
        while g < horizon:
            r = int(np.searchsorted(offsets, g, side='right') - 1)
            end = min(int(offsets[r + 1]), horizon)
            if flags[r]:                                    # a test recording: its hits count, nothing fires
                while i < len(hits) and hits[i] < end:
                    count += 1
                    i += 1
                g = end
                continue
            if count >= self.delay_samples:                 # pushed past by a test recording: fires after this very chunk
                return g                                    # (a hit in it is saved first, and trained on)
            if i < len(hits) and hits[i] < end:
                nxt = int(hits[i])
                count += 1
                i += 1
                if count >= self.delay_samples:
                    return nxt
                g = nxt + 1
            else:
                g = end
        return None


class GeneratedTrainer:
    """The ``fit_generator`` call of ``precise-train-generated`` (scripts/train_generated.py:204-237) over a
    ``generated.Generator``.

    The script's sample stream runs over the background files again and again (the caller shuffles ``files`` once, as the
    script does before its loop); ``samples_to_batches`` cuts it into consecutive batches of ``batch_size`` -- no shuffling,
    across file borders -- and every batch is one optimizer step.  Here the stream is planned ``files_per_plan`` files at a
    time, only when the next batch needs more samples; a plan is mixed and vectorized on the device and its samples go behind
    the trainer's resident training set, where the steps read them by index.  Samples a plan has left over are used before
    the next plan is drawn.  The resident set keeps every sample trained on (n_features x feature_size floats each).

        gen = Generator(runner, backgrounds, positives, negatives)
        history = GeneratedTrainer(trainer, gen).fit(epochs=100, steps_per_epoch=100, batch_size=200, rng=random.Random(1),
                                                     validation_data=(val_in, val_out))

    ``fit`` -> history dict of lists: ``loss`` (the mean of the epoch's batch losses) and, with a validation set (given, or
    already resident), ``val_loss`` / ``val_acc`` measured on the resident validation set after the epoch.  The step counter
    -- and with it the dropout masks -- and the position in the stream run on across epochs and calls."""

    def __init__(self, trainer, generator, replay: str = 'reference', files_per_plan: int = 1):
        self.trainer, self.generator = trainer, generator
        self.replay, self.files_per_plan = replay, max(1, int(files_per_plan))
        self._cursor = 0                # files planned so far: the next one is files[_cursor % len(files)]
        self._next = self._end = 0      # resident samples [_next, _end) are drawn and not yet trained on

    def _more(self, rng, files):
        """plan, load and append the next files of the stream.  A plan may bring no sample (every chunk between the two
        thresholds); sixteen rounds over the files without one end the wait the script would sit out forever"""
        barren = 0
        while True:
            take = [files[(self._cursor + k) % len(files)] for k in range(self.files_per_plan)]
            self._cursor += len(take)
            plan = self.generator.plan(rng, files=take, replay=self.replay)
            if plan.ids.size:
                break
            barren += len(take)
            if barren >= 16 * len(files):
                raise ValueError('%d rounds over the %d background files brought no training sample' % (barren // len(files), len(files)))
        self.generator.load(plan)
        if self._next == self._end:
            self._next = self._end = self.trainer.n_samples()
        self.generator.append_to(self.trainer, plan.ids, plan.targets)
        self._end += int(plan.ids.size)

    def fit(self, epochs, steps_per_epoch, batch_size, rng, validation_data=None, files=None, callback=None) -> dict:
        t, p = self.trainer, self.trainer.params
        batch_size = int(batch_size)
        files = list(range(len(self.generator.backgrounds))) if files is None else [int(f) for f in files]
        if not files or batch_size < 1:
            raise ValueError('fit needs at least one background file and batch_size >= 1')
        if validation_data is not None:
            t.set_data(*validation_data, validation=True)
        validate = t.n_samples(True) > 0
        history = {'loss': []}
        if validate:
            history.update(val_loss=[], val_acc=[])
        for epoch in range(int(epochs)):
            losses = []
            for _ in range(int(steps_per_epoch)):
                while self._end - self._next < batch_size:
                    self._more(rng, files)
                indices = np.arange(self._next, self._next + batch_size)
                self._next += batch_size
                losses.append(t._t.step(indices, dropout_rate=p.dropout, seed=t.seed, step=t._step, loss_bias=p.loss_bias, lr=RMSPROP_LR,
                                        rho=RMSPROP_RHO, eps=RMSPROP_EPS, frozen_mask=t.frozen_mask))
                t._step += 1
            logs = {'loss': float(np.mean(losses))}
            if validate:
                logs['val_loss'], logs['val_acc'] = t._evaluate_resident('validation')
            for k, v in logs.items():
                history[k].append(v)
            if callback is not None:
                callback(epoch, logs)
        return history


# ---- precise-train-sampled (scripts/train_sampled.py) and the samples file of precise-train -sf [-is] -----------------------
def sample_hashes(inputs, outputs) -> list:
    """``calc_sample_hash`` of every row, over the arrays as given (the reference hashes what ``TrainData.load`` returns)"""
    from .util import calc_sample_hash
    return [calc_sample_hash(inp, outp) for inp, outp in zip(inputs, outputs)]


def eligible_mask(hashes) -> np.ndarray:
    """bool [n]: the rows ``hash_to_ind`` points at -- of rows with the same hash the LAST (train.py:116-119)"""
    mask = np.zeros(len(hashes), dtype=bool)
    mask[list({h: i for i, h in enumerate(hashes)}.values())] = True
    return mask


def read_samples_file(path) -> list:
    """The hashes of a samples file in file order, each once: a JSON array of strings or, failing that, one hash per line.
    A missing or empty file is an empty selection."""
    import json
    import os
    if not os.path.isfile(path):
        return []
    with open(path) as f:
        text = f.read()
    try:
        found = json.loads(text) if text.strip() else []
        if not isinstance(found, list):
            raise ValueError('not an array')
    except ValueError:
        found = [line.strip() for line in text.splitlines() if line.strip()]
    return list(dict.fromkeys(str(h) for h in found))


def write_samples_file(path, hashes):
    import json
    with open(path, 'w') as f:
        json.dump(list(hashes), f)


def known_samples(found, hash_to_ind) -> list:
    """``found`` without the hashes the data does not hold, each reported as the reference does (train.py:121-124)"""
    kept = []
    for h in found:
        if h in hash_to_ind:
            kept.append(h)
        else:
            print('Missing hash:', h)
    return kept


def metrics_line(n_selected: int, n: int, n_correct: int) -> str:
    """a line of sampling-metrics.txt (train_sampled.py:55,59)"""
    return '{}\t{}'.format(n_selected / n, float(n_correct / n))


class SampledTrainer:
    """The loop of ``precise-train-sampled`` (scripts/train_sampled.py:72-90) over a ``Trainer`` whose training set stays on
    the device: per cycle ONE ``sample_choose`` -- predict all rows, count, pick at most ``num_sample_chunk`` rows the model
    still gets wrong, all next to the predictions -- and one ``fit_resident(subset=selected)``.  A cycle uploads nothing.

        st = SampledTrainer(trainer, inputs, outputs, num_sample_chunk=50, order='error', validation_data=(val_in, val_out))
        st.load_samples('hey-computer.samples.json')        # continue an earlier run (a missing file: start empty)
        st.run(cycles=200, epochs=1, samples_file='hey-computer.samples.json', metrics_file='sampling-metrics.txt')

    ``order``: which failing rows come first.  The reference takes ``islice`` over a Python set, whose order changes from run
    to run; ``'index'`` (lowest row first) and ``'error'`` (largest float32 ``|p - y|`` first, ties to the lower row) are each
    one legal outcome of it.  Duplicated samples share a hash and the reference's ``hash_to_ind`` keeps the last row: only
    that row is eligible here.  ``hashes`` / ``hash_to_ind``: as the script has them; ``selected``: the chosen rows in order;
    ``samples``: the set of their hashes; ``metrics``: the lines of the metrics file.  ``hashes``: the rows' hashes when
    the caller has them already (default: ``sample_hashes(inputs, outputs)``, once)."""

    def __init__(self, trainer, inputs, outputs, num_sample_chunk: int = 50, order: str = 'index', validation_data=None, hashes=None):
        from ._lib import SAMPLE_MAX_NEW, SAMPLE_ORDER
        if order not in SAMPLE_ORDER:
            raise ValueError("order must be 'index' or 'error', got %r" % (order,))
        if not 0 <= int(num_sample_chunk) <= SAMPLE_MAX_NEW:
            raise ValueError('num_sample_chunk = %d (0..%d rows are chosen per cycle)' % (num_sample_chunk, SAMPLE_MAX_NEW))
        self.trainer, self.num_sample_chunk, self.order = trainer, int(num_sample_chunk), order
        self.hashes = sample_hashes(inputs, outputs) if hashes is None else list(hashes)
        if len(self.hashes) != len(inputs):
            raise ValueError('%d hashes for %d rows' % (len(self.hashes), len(inputs)))
        self.hash_to_ind = {h: i for i, h in enumerate(self.hashes)}
        self.eligible = eligible_mask(self.hashes)
        trainer.set_data(inputs, outputs)
        if validation_data is not None:
            trainer.set_data(*validation_data, validation=True)
        self.n = trainer.n_samples()
        self.metrics = []
        self.samples_file = self.metrics_file = None
        self._reset([])

    def _reset(self, selected):
        self.trainer._t.sample_reset(self.eligible, selected)
        self.selected = [int(i) for i in selected]
        self.samples = {self.hashes[i] for i in self.selected}

    # -- the samples file ---------------------------------------------------------------------------------------------
    def file_indices(self, path, invert=False) -> list:
        """the rows a samples file stands for, in file order; ``invert``: every row of ``hash_to_ind`` NOT in it
        (train.py:150-155), in ascending order"""
        kept = known_samples(read_samples_file(path), self.hash_to_ind)
        if invert:
            return sorted(self.hash_to_ind[h] for h in set(self.hash_to_ind) - set(kept))
        return [self.hash_to_ind[h] for h in kept]

    def load_samples(self, path):
        self._reset(self.file_indices(path))

    def save_samples(self, path):
        write_samples_file(path, [self.hashes[i] for i in self.selected])

    def fit_samples(self, path, invert=False, batch_size=5000, epochs=10, shuffle=True, callback=None) -> dict:
        """``precise-train -sf path [-is]``: fit on the rows of the samples file (``invert``: on all others); the selection
        of this trainer is left alone"""
        rows = self.file_indices(path, invert)
        if not rows:
            raise ValueError('%s selects no sample of this data' % path)
        return self.trainer.fit_resident(batch_size, epochs, shuffle=shuffle, callback=callback, subset=rows)

    # -- the loop -----------------------------------------------------------------------------------------------------
    def cycle(self, epochs, batch_size=5000, shuffle=True) -> dict:
        report, added, _ = self.trainer._t.sample_choose(self.num_sample_chunk, self.order)
        self.selected += [int(i) for i in added]
        self.samples.update(self.hashes[i] for i in added)
        self.metrics.append(metrics_line(len(self.samples), report['n'], report['n_correct']))
        if self.samples_file:
            self.save_samples(self.samples_file)
        if self.metrics_file:
            with open(self.metrics_file, 'w') as f:
                f.write('\n'.join(self.metrics))
        history = None
        if self.selected:
            history = self.trainer.fit_resident(batch_size, epochs, shuffle=shuffle, subset=self.selected)
        return {'remaining': report['n_remaining'], 'added': [int(i) for i in added], 'correct': float(report['n_correct'] / report['n']),
                'ratio': len(self.samples) / report['n'], 'history': history}

    def run(self, cycles, epochs, batch_size=5000, samples_file=None, metrics_file=None, callback=None) -> list:
        """``cycles`` cycles; the samples file and the metrics file, when given, are rewritten after every choice, before
        the fit, as the script does.  ``callback(cycle, result)`` runs after every cycle.  -> the cycles' results"""
        self.samples_file, self.metrics_file = samples_file, metrics_file
        results = []
        try:
            for c in range(int(cycles)):
                results.append(self.cycle(epochs, batch_size))
                if callback is not None:
                    callback(c, results[-1])
        finally:
            self.samples_file = self.metrics_file = None
        return results


def fit_samples(trainer, inputs, outputs, path, invert=False, **fit_args) -> dict:
    """``precise-train -sf path [-is]`` in one call: one upload, then ``fit_resident`` over the file's rows"""
    return SampledTrainer(trainer, inputs, outputs).fit_samples(path, invert, **fit_args)
