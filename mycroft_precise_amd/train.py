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

``TrainerGroup`` trains several candidate networks -- other widths, dropout rates, ``loss_bias`` values, seeds -- on the same
data at once: one resident dataset, one launch per batch for all of them, and each candidate ends with exactly the bits that a
``Trainer`` of its own would have given it.

    group = TrainerGroup([ModelParams(recurrent_units=u, loss_bias=b) for u in (12, 20, 32) for b in (0.5, 0.7)])
    histories = group.fit(inputs, outputs, validation_data=(val_in, val_out))
    group.save(group.best('val_loss'), 'hey-computer.npz')

There is no CPU fallback: without the HIP library or a GPU the constructor raises.
"""
import numpy as np

from ._lib import HipTrainer, dropout_masks            # noqa: F401  (dropout_masks: the kernel's mask function on the host)
from .model import ModelParams, create_model, save_weights
from .params import pr, save_params

# keras.optimizers.RMSprop defaults of Keras 2.2.4 (what compile('rmsprop') builds)
RMSPROP_LR, RMSPROP_RHO, RMSPROP_EPS = 1e-3, 0.9, 1e-7


def flatten_weights(weights: dict) -> np.ndarray:
    """weights dict (one GRU layer) -> the trainer's flat float32 vector: kernel | recurrent_kernel | bias | dense_kernel |
    dense_bias."""
    (k, rk, b), = weights['gru']
    parts = [k, rk, b, weights['dense_kernel'], weights['dense_bias']]
    return np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in parts])


def unflatten_weights(flat, feature_size: int, units: int) -> dict:
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    F, H = int(feature_size), int(units)
    sizes = [F * 3 * H, H * 3 * H, 3 * H, H, 1]
    if flat.size != sum(sizes):
        raise ValueError('expected %d values for F = %d, H = %d, got %d' % (sum(sizes), F, H, flat.size))
    k, rk, b, dk, db = np.split(flat, np.cumsum(sizes)[:-1])
    return {'gru': [(k.reshape(F, 3 * H).copy(), rk.reshape(H, 3 * H).copy(), b.copy())],
            'dense_kernel': dk.reshape(H, 1).copy(), 'dense_bias': db.copy()}


class Trainer:
    """``weights``: a weights dict to continue from; None = ``create_model``'s random network for the current ``pr`` and
    ``params.recurrent_units``.  ``params`` supplies ``dropout``, ``loss_bias`` (the reference passes ``1.0 - sensitivity``,
    scripts/train.py:86) and ``freeze_till``.  ``seed`` drives the initial network, the shuffle and the dropout masks."""

    def __init__(self, weights=None, params: ModelParams = None, seed: int = 42, device: int = 0, n_features: int = None):
        self.params = params or ModelParams()
        self.seed = int(seed)
        if weights is None:
            weights = create_model(None, self.params, seed=self.seed)
        if len(weights['gru']) != 1:
            raise NotImplementedError('training: n_layers = %d (one GRU layer has a training kernel)' % len(weights['gru']))
        k, rk, _ = weights['gru'][0]
        self.feature_size, self.units = int(np.shape(k)[0]), int(np.shape(rk)[0])
        self.n_features = int(pr.n_features if n_features is None else n_features)
        self._t = HipTrainer(weights, self.n_features, self.feature_size, device=device)
        self._rng = np.random.default_rng(self.seed)
        self._step = 0                   # optimizer steps taken so far: the dropout masks' step counter
        self.frozen_mask = ((1 << max(0, int(self.params.freeze_till))) - 1) & 3      # model.py:84-85: layers[:freeze_till]

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
        [3, N, feature_size] per-gate input dropout masks or None.  Changes no state."""
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
        p = self.params
        history = {'loss': [], 'acc': []}
        if validation_data is not None:
            history.update(val_loss=[], val_acc=[])
        for epoch in range(int(epochs)):
            order = self._rng.permutation(n) if shuffle else np.arange(n)
            losses = []
            for a in range(0, n, int(batch_size)):
                losses.append(self._t.step(order[a:a + int(batch_size)], dropout_rate=p.dropout, seed=self.seed, step=self._step,
                                           loss_bias=p.loss_bias, lr=RMSPROP_LR, rho=RMSPROP_RHO, eps=RMSPROP_EPS,
                                           frozen_mask=self.frozen_mask))
                self._step += 1
            logs = {'loss': float(np.mean(losses)), 'acc': self.evaluate(inputs, outputs)[1]}
            if validation_data is not None:
                logs['val_loss'], logs['val_acc'] = self.evaluate(*validation_data)
            for k, v in logs.items():
                history[k].append(v)
            if callback is not None:
                callback(epoch, logs)
        return history

    def close(self):
        self._t.close()


class TrainerGroup:
    """K candidate networks trained together on ONE resident dataset (``pe_trainer_create_models``).

    ``candidates``: a list of ``ModelParams``; ``recurrent_units``, ``dropout``, ``loss_bias`` and ``freeze_till`` mean what
    they mean to ``Trainer``.  ``seeds[m]`` (default: ``seed`` for every candidate) drives candidate m's initial network and its
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
        for w in weights:
            if len(w['gru']) != 1:
                raise NotImplementedError('training: n_layers = %d (one GRU layer has a training kernel)' % len(w['gru']))
        sizes = {int(np.shape(w['gru'][0][0])[0]) for w in weights}
        if len(sizes) != 1:
            raise ValueError('the candidates of a group share feature_size, got %s' % sorted(sizes))
        self.feature_size = sizes.pop()
        self.units = [int(np.shape(w['gru'][0][1])[0]) for w in weights]
        self.n_features = int(pr.n_features if n_features is None else n_features)
        self._t = HipTrainer(weights, self.n_features, self.feature_size, device=device)
        self._rng = np.random.default_rng(self.seed)
        self._step = 0
        self.frozen_masks = [((1 << max(0, int(p.freeze_till))) - 1) & 3 for p in self.candidates]

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

    def best(self, key: str = 'val_loss') -> int:
        """the candidate whose last-epoch ``key`` is smallest (largest for the accuracies)"""
        if not getattr(self, 'histories', None) or key not in self.histories[0] or not self.histories[0][key]:
            raise ValueError('no %r in the histories of this group (call fit first)' % key)
        last = [h[key][-1] for h in self.histories]
        return int(np.argmax(last) if key.endswith('acc') else np.argmin(last))

    def close(self):
        self._t.close()
