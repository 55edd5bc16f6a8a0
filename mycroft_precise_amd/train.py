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
