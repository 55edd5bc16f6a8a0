"""CPU: pe_create_models / MultiModelListener refuse what one engine cannot hold -- before any device work."""
import ctypes as C

import numpy as np
import pytest

from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.params import pr


def _create_models(models, n_models=None):
    """pe_create_models through ctypes with an explicit count (the wrapper always passes len(models))."""
    lib = _lib.load()
    keep = []
    ws = (_lib.PeWeights * max(1, len(models)))()
    for m, w in enumerate(models):
        layers = (_lib.PeGruLayer * len(w['gru']))()
        for i, (k, rk, b) in enumerate(w['gru']):
            k, rk, b = (np.ascontiguousarray(x, dtype=np.float32) for x in (k, rk, b))
            keep += [k, rk, b]
            layers[i] = _lib.PeGruLayer(k.shape[0], rk.shape[0], _lib._fptr(k), _lib._fptr(rk), _lib._fptr(b))
        dk = np.ascontiguousarray(w['dense_kernel'], dtype=np.float32).reshape(-1)
        keep += [layers, dk]
        ws[m] = _lib.PeWeights(len(w['gru']), layers, _lib._fptr(dk), float(np.asarray(w['dense_bias']).reshape(-1)[0]))
    p = _lib.PeParams(pr.sample_rate, pr.window_samples, pr.hop_samples, pr.n_fft, pr.n_filt, pr.n_mfcc, pr.n_features,
                      0, 0, 0, 2, 0)
    mel = np.zeros((pr.n_filt, pr.n_fft // 2 + 1), dtype=np.float64)
    h = C.c_void_p()
    rc = lib.pe_create_models(C.byref(p), mel.ctypes.data_as(C.POINTER(C.c_double)), ws,
                              len(models) if n_models is None else n_models, 4, 0, C.byref(h))
    return rc, lib.pe_last_global_error().decode()


def test_model_count_is_checked():
    w = synth.make_weights()
    rc, msg = _create_models([w], n_models=0)
    assert rc == _lib.PE_ERR_INVALID and 'n_models' in msg
    rc, msg = _create_models([w] * 9)
    assert rc == _lib.PE_ERR_INVALID and 'n_models' in msg


@pytest.mark.parametrize('other,field', [
    (synth.make_weights(units=(16,), seed=3), 'units'),
    (synth.make_weights(units=(20, 20), seed=3), 'n_layers'),
    (synth.make_weights(n_in=26, seed=3), 'n_in'),
])
def test_mismatched_architecture_is_refused_by_model_and_field(other, field):
    w = synth.make_weights()
    rc, msg = _create_models([w, w, other])
    assert rc == _lib.PE_ERR_UNSUPPORTED, msg
    assert 'model 2' in msg and field in msg, msg
    with pytest.raises(NotImplementedError, match='model 2'):
        _lib.HipEngine(pr, [w, w, other], n_streams=4)


def test_multi_model_listener_refuses_different_front_ends():
    from mycroft_precise_amd.network_runner import MultiModelListener
    w = synth.make_weights()
    other = pr.copy()
    other.__dict__['hop_t'] = 0.025
    assert other.hop_samples != pr.hop_samples
    import mycroft_precise_amd.network_runner as nr
    real = nr.inject_params
    try:
        nr.inject_params = lambda name: other if name == 'b.net' else pr
        nr_load = nr.load_weights
        nr.load_weights = lambda name: w
        with pytest.raises(ValueError, match=r'model 1 \(b.net\): hop_samples'):
            MultiModelListener(['a.net', 'b.net'], n_streams=4)
    finally:
        nr.inject_params = real
        nr.load_weights = nr_load
    with pytest.raises(ValueError):
        MultiModelListener([], n_streams=4)


def test_header_declares_the_multi_model_entry_points():
    for name in ('pe_create_models', 'pe_get_n_models', 'pe_set_decoder_model', 'pe_set_trigger_model'):
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 8
