"""CPU: the C ABI declares the stacked trainer constructor (one or two GRU layers of 1..256 units) and the
per-layer mask function; the refusals happen before any device work and name what they refuse; the flat layout round-trips;
and the float64 reference the GPU tests lean on (train_stacked_reference.py) checks out against the oracle."""
import ctypes
import os
import re

import numpy as np
import pytest

import train_stacked_reference as ref
from conftest import REPO
from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.model import ModelParams
from mycroft_precise_amd.train import flatten_weights, unflatten_weights
from test_train_wide_host import created_or_no_device


def test_stacked_entry_points_are_declared_and_bound():
    text = open(os.path.join(REPO, 'include', 'precise_engine.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (('pe_trainer_create_stacked', 6), ('pe_train_dropout_masks_layer', 7)):
        m = re.search(r'\b%s\s*\(([^)]*)\)' % name, code)
        assert m, 'the header does not declare ' + name
        assert name in _lib.EXPORTS and len(_lib.EXPORTS[name][1]) == m.group(1).count(',') + 1 == n_args
        assert hasattr(raw, name), 'library does not export ' + name
    assert _lib.EXPORTS['pe_trainer_create_stacked'] == _lib.EXPORTS['pe_trainer_create_wide']


def test_stacked_refusals_need_no_gpu():
    """by name and before any device work (this machine may have no GPU at all)"""
    one, two = synth.make_weights(13, (20,)), synth.make_weights(13, (64, 64))
    cap = _lib.TRAIN_MAX_MODELS
    with pytest.raises(NotImplementedError, match=r'^training: n_layers = 3 \(1\.\.2\)'):
        _lib.HipTrainer(synth.make_weights(13, (20, 20, 20)), 29, 13, stacked=True)
    with pytest.raises(NotImplementedError, match=r'^training: units = 257 \(1\.\.256\)'):
        _lib.HipTrainer(synth.make_weights(13, (257, 20)), 29, 13, stacked=True)
    with pytest.raises(NotImplementedError, match=r'^training: units = 257 \(1\.\.256\)'):
        _lib.HipTrainer(synth.make_weights(13, (20, 257)), 29, 13, stacked=True)
    with pytest.raises(NotImplementedError, match=r'^training: units = 257'):
        _lib.HipTrainer(synth.make_weights(13, (257,)), 29, 13, stacked=True)
    crooked = dict(two, gru=[two['gru'][0], synth.make_weights(63, (64,))['gru'][0]])
    with pytest.raises(ValueError, match=r'^GRU layer 1 takes 63 inputs, layer 0 has 64 units'):
        _lib.HipTrainer(crooked, 29, 13, stacked=True)
    with pytest.raises(ValueError, match=r'takes 12 inputs, feature_size is 13'):
        _lib.HipTrainer(synth.make_weights(12, (64, 64)), 29, 13, stacked=True)
    with pytest.raises(NotImplementedError, match=r'^training: n_features = 65'):
        _lib.HipTrainer(two, 65, 13, stacked=True)
    with pytest.raises(NotImplementedError, match='n_models = %d' % (cap + 1)):
        _lib.HipTrainer([two] * (cap + 1), 29, 13, stacked=True)
    with pytest.raises(ValueError, match='n_models'):
        _lib.HipTrainer([], 29, 13, stacked=True)
    # "model i: " in a mixed list
    with pytest.raises(NotImplementedError, match=r'^model 2: training: n_layers = 3'):
        _lib.HipTrainer([one, two, synth.make_weights(13, (20, 20, 20))], 29, 13, stacked=True)
    with pytest.raises(NotImplementedError, match=r'^model 1: training: units = 257'):
        _lib.HipTrainer([two, synth.make_weights(13, (64, 257)), one], 29, 13, stacked=True)
    with pytest.raises(ValueError, match=r'^model 0: GRU layer 1 takes 63 inputs'):
        _lib.HipTrainer([crooked, one], 29, 13, stacked=True)
    # the older constructors keep refusing two layers
    for kwargs in ({}, {'wide': True}):
        with pytest.raises(NotImplementedError, match='n_layers'):
            _lib.HipTrainer(two, 29, 13, **kwargs)


def test_stacked_null_entries_are_invalid():
    lib = _lib.load()
    h = ctypes.c_void_p()
    ws = (_lib.PeWeights * 2)()                 # zeroed: null layer arrays
    ws[0].n_layers, ws[1].n_layers = 2, 1
    assert lib.pe_trainer_create_stacked(29, 13, ws, 2, 0, ctypes.byref(h)) == _lib.PE_ERR_INVALID
    assert b'model 0' in lib.pe_trainer_last_error(None) and not h.value
    # layer 0 whole, layer 1's arrays null
    w, keep = _lib._pe_weights(synth.make_weights(13, (20, 20)))
    layers = (_lib.PeGruLayer * 2)()
    layers[0] = w.layers[0]
    layers[1].n_in, layers[1].units = 20, 20
    one = (_lib.PeWeights * 1)()
    one[0] = _lib.PeWeights(2, layers, w.dense_kernel, w.dense_bias)
    assert lib.pe_trainer_create_stacked(29, 13, one, 1, 0, ctypes.byref(h)) == _lib.PE_ERR_INVALID
    assert b'null weight array' in lib.pe_trainer_last_error(None) and not h.value
    assert lib.pe_trainer_create_stacked(29, 13, None, 2, 0, ctypes.byref(h)) == _lib.PE_ERR_INVALID
    assert lib.pe_trainer_create_stacked(29, 13, ws, 2, 0, None) == _lib.PE_ERR_INVALID
    del keep


def test_a_valid_stacked_trainer_is_created_where_the_library_runs():
    """without a GPU the creation fails with the HIP error, not with a refusal"""
    mixed = [synth.make_weights(13, (40, 200)), synth.make_weights(13, (20,)), synth.make_weights(13, (256, 256))]
    t = created_or_no_device(lambda: _lib.HipTrainer(mixed, 29, 13, stacked=True))
    if t is not None:
        n = lambda F, H: (F + H + 1) * 3 * H         # noqa: E731
        assert t.n_params == [n(13, 40) + n(40, 200) + 201, n(13, 20) + 21, n(13, 256) + n(256, 256) + 257]
        assert t.n_params_total == sum(t.n_params) and t.units == [(40, 200), 20, (256, 256)]
        t.close()
    from mycroft_precise_amd.train import Trainer, TrainerGroup
    tr = created_or_no_device(lambda: Trainer(params=ModelParams(recurrent_units=(24, 16), freeze_till=3)))
    if tr is not None:
        assert tr.units == (24, 16) and tr.frozen_mask == 7
        tr.close()
    group = created_or_no_device(lambda: TrainerGroup([ModelParams(recurrent_units=u, freeze_till=3) for u in (20, (24, 16))]))
    if group is not None:
        assert group.units == [20, (24, 16)] and group.frozen_masks == [3, 7]
        group.close()


@pytest.mark.parametrize('rate', [0.0, 0.2, 0.5])
@pytest.mark.parametrize('width', [1, 13, 32, 33, 256])
def test_mask_function_of_both_layers(width, rate):
    """pe_train_dropout_masks_layer against the numpy restatement of the header's description; layer 0 (widths up to 32) is
    pe_train_dropout_masks in bytes"""
    n, seed, step = 37, 0xFEDCBA9876543210, 7
    got = _lib.dropout_masks(seed, step, n, width, rate, layer=1)
    assert got.tobytes() == ref.mask_function(seed, step, n, width, rate, layer=1).tobytes()
    assert set(np.unique(got)) <= {np.float32(0.0), np.float32(1.0) / (np.float32(1.0) - np.float32(rate))}
    if rate > 0 and width >= 13:
        assert 0.5 * rate < float((got == 0).mean()) < 1.5 * rate
    lib = _lib.load()
    if width <= 32:
        layer0 = np.empty((3, n, width), dtype=np.float32)
        assert lib.pe_train_dropout_masks_layer(seed, step, 0, n, width, rate, layer0.ctypes.data) == _lib.PE_OK
        assert layer0.tobytes() == _lib.dropout_masks(seed, step, n, width, rate).tobytes()
        assert layer0.tobytes() == ref.mask_function(seed, step, n, width, rate, layer=0).tobytes()
        if rate > 0 and width >= 13:
            assert layer0.tobytes() != got.tobytes()
    else:
        out = np.full((3, n, width), 7.0, dtype=np.float32)
        assert lib.pe_train_dropout_masks_layer(seed, step, 0, n, width, rate, out.ctypes.data) == _lib.PE_ERR_INVALID
        assert np.all(out == 7.0)


def test_mask_function_refusals():
    with pytest.raises(ValueError, match=r'layer = 2'):
        _lib.dropout_masks(0, 0, 4, 13, 0.2, layer=2)
    with pytest.raises(ValueError, match=r'width = 257'):
        _lib.dropout_masks(0, 0, 4, 257, 0.2, layer=1)
    with pytest.raises(ValueError, match='outside'):
        _lib.dropout_masks(0, 0, 4, 64, 1.0, layer=1)
    with pytest.raises(ValueError):
        _lib.dropout_masks(0, 0, 0, 64, 0.2, layer=1)


@pytest.mark.parametrize('units', [(20,), (64,), (20, 20), (40, 200)])
def test_flat_layout_round_trips(units):
    w = synth.make_weights(13, units)
    flat = flatten_weights(w)
    sizes, n_in = 0, 13
    for H in units:
        sizes += (n_in + H + 1) * 3 * H
        n_in = H
    assert flat.dtype == np.float32 and flat.size == sizes + units[-1] + 1
    # the order: layer by layer, kernel | recurrent_kernel | bias, then the dense layer
    assert np.array_equal(flat[:13 * 3 * units[0]], w['gru'][0][0].reshape(-1))
    assert np.array_equal(flat[-units[-1] - 1:-1], w['dense_kernel'].reshape(-1)) and flat[-1] == w['dense_bias'][0]
    if len(units) == 2:
        o = (13 + units[0] + 1) * 3 * units[0]
        assert np.array_equal(flat[o:o + units[0] * 3 * units[1]], w['gru'][1][0].reshape(-1))
    back = unflatten_weights(flat, 13, units if len(units) == 2 else units[0])
    assert len(back['gru']) == len(units)
    for got, want in zip(back['gru'], w['gru']):
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a, b)
    assert np.array_equal(back['dense_kernel'], w['dense_kernel']) and np.array_equal(back['dense_bias'], w['dense_bias'])
    assert np.array_equal(flatten_weights(back), flat)
    for wrong in (flat[:-1], np.concatenate([flat, flat[:1]])):
        with pytest.raises(ValueError, match='expected %d values' % flat.size):
            unflatten_weights(wrong, 13, units if len(units) == 2 else units[0])


def test_create_model_passes_a_tuple_through():
    from mycroft_precise_amd.model import create_model
    w = create_model(None, ModelParams(recurrent_units=(24, 16)), seed=3)
    assert [rk.shape for _, rk, _ in w['gru']] == [(24, 72), (16, 48)] and w['dense_kernel'].shape == (16, 1)
    want = synth.make_weights(13, (24, 16), seed=3)
    assert all(np.array_equal(a, b) for la, lb in zip(w['gru'], want['gru']) for a, b in zip(la, lb))
    one = create_model(None, ModelParams(recurrent_units=24), seed=3)
    assert len(one['gru']) == 1 and one['gru'][0][1].shape == (24, 72)


@pytest.mark.parametrize('units', [(20, 20), (40, 200), (64,)])
def test_reference_forward_equals_the_oracle(units):
    """dropout-free, against oracle.keras_gru.predict in float64 (to rounding) and in float32 (to the float32 floor)"""
    from oracle import keras_gru
    w = synth.make_weights(13, units)
    x = np.random.default_rng(1).normal(0.0, 1.0, (24, 29, 13)).astype(np.float32)
    got = ref.forward_numpy(w, x)['p']
    assert float(np.abs(got - keras_gru.predict(x, w, dtype=np.float64).reshape(-1)).max()) <= 1e-12
    assert float(np.abs(got - keras_gru.predict(x, w, dtype=np.float32).reshape(-1)).max()) <= 1e-5
    if len(units) == 1:
        import train_reference
        one = train_reference.loss_and_grads(w, x, np.ones(24), None, 0.7)
        two = ref.loss_and_grads(w, x, np.ones(24), None, 0.7)
        assert one['loss'] == two['loss'] and np.array_equal(train_reference.flat_grads(one), ref.flat_grads(two))


def test_reference_layer0_gradients_vanish_behind_a_dead_layer1():
    """layer 1's kernel zeroed: nothing of layer 0 reaches the loss, so layer 0's gradients are exact zeros while layer 1's
    recurrent part and the dense layer still have theirs"""
    w = synth.make_weights(13, (20, 24))
    k1, rk1, b1 = w['gru'][1]
    dead = dict(w, gru=[w['gru'][0], (np.zeros_like(k1), rk1, b1)])
    x = np.random.default_rng(2).normal(0.0, 1.0, (9, 5, 13)).astype(np.float32)
    y = (np.arange(9) % 2).astype(np.float32)
    masks = (_lib.dropout_masks(1, 2, 9, 13, 0.2), _lib.dropout_masks(1, 2, 9, 20, 0.2, layer=1))
    res = ref.loss_and_grads(dead, x, y, masks, 0.7)
    for name in ('kernel_0', 'recurrent_kernel_0', 'bias_0'):
        assert not res['grads'][name].any(), name
    for name in ('kernel_1', 'recurrent_kernel_1', 'bias_1', 'dense_kernel', 'dense_bias'):
        assert res['grads'][name].any(), name
    live = ref.loss_and_grads(w, x, y, masks, 0.7)
    assert all(live['grads'][name].any() for name in ('kernel_0', 'recurrent_kernel_0', 'bias_0'))
    # layer 1's masks matter: without them the loss differs
    assert live['loss'] != ref.loss_and_grads(w, x, y, (masks[0], None), 0.7)['loss']
