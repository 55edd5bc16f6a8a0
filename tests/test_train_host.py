"""CPU: the float64 training reference is pinned to the oracle and to finite differences, the C ABI declares the trainer,
and the dropout-mask function (host arithmetic, no GPU) is the documented one."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import train_reference as ref
from conftest import REPO
from mycroft_precise_amd import _lib, synth
from oracle import keras_gru

TRAINER_SYMBOLS = ('pe_trainer_create', 'pe_trainer_destroy', 'pe_trainer_last_error', 'pe_trainer_get_weights',
                   'pe_trainer_set_weights', 'pe_trainer_loss_grad', 'pe_trainer_apply', 'pe_trainer_reset_optimizer',
                   'pe_trainer_set_data', 'pe_trainer_step', 'pe_trainer_evaluate', 'pe_train_dropout_masks')


def test_reference_forward_is_the_oracle(stock_weights):
    x = np.random.default_rng(0).normal(0.0, 1.0, (64, 29, 13))
    want = keras_gru.predict(x, stock_weights, dtype=np.float64).reshape(-1)
    with torch.no_grad():
        got = ref.forward(ref.tensors(stock_weights, requires_grad=False), x)['p'].numpy()
    err = float(np.abs(got - want).max())
    print('reference forward vs oracle float64: %.3g' % err)
    assert err <= 1e-12


def test_reference_gradients_match_finite_differences(stock_weights):
    rng = np.random.default_rng(1)
    x = rng.normal(0.0, 1.0, (64, 29, 13))
    masks = ref.mask_function(3, 0, 64, 13, 0.2)
    # samples far enough from every kink that a 1e-6 step cannot cross one
    keep = ref.pick_kink_safe(stock_weights, x, masks, delta=1e-3)
    assert keep.size >= 32
    x, masks = x[keep], masks[:, keep]
    y = (rng.random(keep.size) < 0.5).astype(np.float64)
    res = ref.loss_and_grads(stock_weights, x, y, masks, 0.7)
    params = ref.tensors(stock_weights, requires_grad=False)
    h = 1e-6
    worst = 0.0
    for _ in range(40):
        ti = int(rng.integers(len(params)))
        flat = params[ti].view(-1)
        ei = int(rng.integers(flat.numel()))
        old = float(flat[ei])
        with torch.no_grad():
            flat[ei] = old + h
            up = float(ref.loss_fn(params, x, y, masks, 0.7)[0])
            flat[ei] = old - h
            down = float(ref.loss_fn(params, x, y, masks, 0.7)[0])
            flat[ei] = old
        fd = (up - down) / (2 * h)
        an = float(res['grads'][ref.NAMES[ti]].reshape(-1)[ei])
        scale = float(np.abs(res['grads'][ref.NAMES[ti]]).max())
        worst = max(worst, abs(fd - an) / scale)
    print('autograd vs central differences, relative to the tensor: %.3g' % worst)
    assert worst <= 1e-6


def test_trainer_abi_is_declared_and_bound():
    text = open(os.path.join(REPO, 'include', 'precise_engine.h')).read()
    assert re.search(r'#define\s+PE_ABI_VERSION\s+8\b', text) and _lib.ABI_VERSION == 8
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in TRAINER_SYMBOLS:
        m = re.search(r'\b%s\s*\(([^)]*)\)' % name, code)
        assert m, 'the header does not declare ' + name
        n_args = 0 if m.group(1).strip() in ('', 'void') else m.group(1).count(',') + 1
        assert name in _lib.EXPORTS, name
        assert len(_lib.EXPORTS[name][1]) == n_args, name
        assert hasattr(raw, name), 'library does not export ' + name
    assert 'typedef struct pe_trainer pe_trainer;' in code


@pytest.mark.parametrize('rate', [0.0, 0.2, 0.5])
@pytest.mark.parametrize('F', [13, 26])
@pytest.mark.parametrize('n', [1, 17, 5000])
def test_dropout_masks_are_the_documented_function(n, F, rate):
    got = _lib.dropout_masks(1234, 7, n, F, rate)
    want = ref.mask_function(1234, 7, n, F, rate)
    assert got.shape == (3, n, F) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    kept = np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
    assert np.all((got == 0.0) | (got == kept))
    if n == 5000:
        for g in range(3):
            assert abs(float((got[g] != 0).mean()) - (1.0 - rate)) <= 0.02
    if rate > 0 and n > 1:
        assert not np.array_equal(got, _lib.dropout_masks(1234, 8, n, F, rate))
        assert not np.array_equal(got, _lib.dropout_masks(1235, 7, n, F, rate))
        assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])


def test_dropout_masks_argument_errors():
    for bad in (1.0, -0.1, float('nan')):
        with pytest.raises(ValueError):
            _lib.dropout_masks(0, 0, 4, 13, bad)
    with pytest.raises(ValueError):
        _lib.dropout_masks(0, 0, 0, 13, 0.2)


def test_trainer_refusals_need_no_gpu():
    """Shapes without a training kernel are refused by name before any device work."""
    for weights, T, F, field in ((synth.make_weights(13, (20, 20)), 29, 13, 'n_layers'),
                                 (synth.make_weights(13, (33,)), 29, 13, 'units'),
                                 (synth.make_weights(13, (20,)), 65, 13, 'n_features'),
                                 (synth.make_weights(33, (20,)), 29, 33, 'feature_size')):
        with pytest.raises(NotImplementedError, match=field):
            _lib.HipTrainer(weights, T, F)
