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


def head64(p, y, beta=0.7):
    """ds N of DESIGN.md 4.9 in Python floats (float64) at a given p"""
    return (beta * (1 - y) / (1 - p + 1e-7) - (1 - beta) * y / (p + 1e-7)) * p * (1 - p)


def sigmoid32(logit):
    """the float32 nearest the float64 sigmoid, as a Python float: both heads are functions of p and get the SAME p (at logit 8
    with y = 1, ds is proportional to 1 - p = 3.4e-4, which the rounding of p alone moves by 4e-5 relative)"""
    return np.float32(1.0 / (1.0 + np.exp(-np.asarray(logit, dtype=np.float64)))).astype(np.float64)


def test_head32_matches_float64_off_the_positive_side():
    for L in (-30.0, -19.0, -12.0, -8.0, -3.0, 0.0, 0.5, 8.0):
        for y in (0.0, 1.0):
            p = float(sigmoid32(L))
            d64 = head64(p, y)
            ds, neg, pos = ref.head32(np.float32(p), np.float32(y), 0.7, 1)
            assert abs(ds - d64) <= 1e-6 * abs(d64), (L, y, ds, d64)
            assert abs(neg - -(1 - y) * np.log(1 - p + 1e-7)) <= 1e-6 and abs(pos - -y * np.log(p + 1e-7)) <= 1e-6 * max(1.0, pos)
    # a batch: the means divide by n, in float32
    p = sigmoid32(np.linspace(-30.0, 8.0, 77))
    y = (np.arange(77) % 2).astype(np.float64)
    ds = ref.head32(p.astype(np.float32), y.astype(np.float32), 0.7, 77)[0]
    assert ds.shape == (77,) and ds.dtype == np.float64
    assert np.all(np.abs(ds * 77 - head64(p, y)) <= 1e-6 * np.abs(head64(p, y)))


def test_head32_is_zero_at_p_one():
    for y in (0.0, 1.0):
        for beta in (0.7, 0.0, 1.0):
            ds, neg, pos = ref.head32(np.float32(1.0), np.float32(y), beta, 1)
            assert ds == 0.0 and np.isfinite(neg) and np.isfinite(pos)
            # the loss terms at q == eps and pe == fl(1 + eps)
            assert neg == -(1 - y) * np.log(float(np.float32(1e-7)))
            assert pos == -y * np.log(float(np.float32(1.0) + np.float32(1e-7)))
    ds = ref.head32(np.ones(5, dtype=np.float32), np.array([0, 1, 0, 1, 1], dtype=np.float32), 0.7, 5)[0]
    assert not ds.any()
    # and at p == 0 (a logit below -88.7, where the float32 exp overflows): no 0 inf either
    assert ref.head32(np.float32(0.0), np.float32(1.0), 0.7, 1)[0] == 0.0


def test_head32_beyond_logit_12_is_its_own_contract():
    """The table of DESIGN.md 4.9: at logits 12, 14 and 16 with y = 0 the float32 head leaves the float64 head by 1e-5, 4e-4
    and 3 %, and one ulp of p moves it by up to 30 %.  The expected values are the formula in Python floats on float32-rounded
    operands, rounded after every operation."""
    f = np.float32
    for L, apart, ulp_moves in ((12.0, 1e-6, 1e-4), (14.0, 1e-4, 5e-3), (16.0, 1e-2, 0.1)):
        p = f(1.0 / (1.0 + np.exp(-L)))
        below, above = np.nextafter(p, f(0.0)), np.nextafter(p, f(2.0))
        got = [float(ref.head32(v, f(0.0), 0.7, 1)[0]) for v in (below, p, above)]
        want = []
        for v in (below, p, above):
            q = float(f(float(f(1.0 - float(v))) + float(f(1e-7))))                      # 1 - p is exact in float32 (Sterbenz)
            dp = float(f(float(f(0.7)) / q))
            want.append(float(f(float(f(dp * float(v))) * float(f(1.0 - float(v))))))
        assert got == want, (L, got, want)
        d64 = head64(1.0 / (1.0 + np.exp(-L)), 0.0)                              # (here p in float64: the table's first column)
        assert abs(got[1] - d64) > apart * d64                                   # float64 is no reference here ...
        assert got[0] - got[2] > ulp_moves * d64                                 # ... and p must be the kernel's own
    assert float(ref.head32(f(1.0 / (1.0 + np.exp(-8.0))), f(0.0), 0.7, 1)[0]) == pytest.approx(head64(1.0 / (1.0 + np.exp(-8.0)), 0.0), rel=1e-6)


def test_logit_bands():
    logit = np.array([-50.0, -19.0, -18.99, -8.0, -7.99, 0.0, 7.99, 8.0, 16.99, 17.0, 18.99, 19.0, 60.0])
    want = ['neg_sat', 'neg_sat', 'neg', 'neg', 'mid', 'mid', 'mid', 'pos', 'pos', 'edge', 'edge', 'one', 'one']
    assert list(ref.logit_bands(logit)) == want and set(want) == set(ref.BANDS)
    # what the bands promise about the float32 sigmoid
    sig = 1.0 / (1.0 + np.exp(-np.array([19.0, 16.99])))
    assert 1.0 - sig[0] < 2.0 ** -25 and np.float32(sig[0]) == np.float32(1.0) and np.float32(sig[1]) < np.float32(1.0)


def test_grads_from_ds_is_the_backward_pass_of_the_reference(stock_weights):
    rng = np.random.default_rng(4)
    x = rng.normal(0.0, 1.0, (64, 29, 13))
    masks = ref.mask_function(5, 0, 64, 13, 0.2)
    keep = ref.pick_kink_safe(stock_weights, x, masks)
    assert keep.size >= 32
    x, masks = x[keep], masks[:, keep]
    y = (rng.random(keep.size) < 0.5).astype(np.float64)
    res = ref.loss_and_grads(stock_weights, x, y, masks, 0.7)
    p, n = res['p'], keep.size
    ds = (0.7 * (1 - y) / (1 - p + ref.EPS) - 0.3 * y / (p + ref.EPS)) / n * p * (1 - p)
    got = ref.grads_from_ds(stock_weights, x, masks, ds)
    for name in ref.NAMES:
        want = res['grads'][name]
        assert got[name].shape == want.shape
        err = float(np.abs(got[name] - want).max() / np.abs(want).max())
        print('%s: %.3g' % (name, err))
        assert err <= 1e-12
    # the float32 head on that batch (|logit| <= 8) is the float64 head to 1e-6
    ds32 = ref.head32(p.astype(np.float32), y.astype(np.float32), 0.7, n)[0]
    assert np.all(np.abs(ds32 - ds) <= 1e-6 * np.abs(ds))
    assert abs(ref.head32_loss(p.astype(np.float32), y.astype(np.float32), 0.7) - res['loss']) <= 1e-6


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
