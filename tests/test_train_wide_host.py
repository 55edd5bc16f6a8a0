"""CPU: the C ABI declares the wide trainer constructor (networks of up to 256 units), its refusals happen
before any device work and name what they refuse, and ``Trainer`` no longer stops at 32 units."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.model import ModelParams


def test_wide_constructor_is_declared_and_bound():
    text = open(os.path.join(REPO, 'include', 'precise_engine.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    name = 'pe_trainer_create_wide'
    m = re.search(r'\b%s\s*\(([^)]*)\)' % name, code)
    assert m, 'the header does not declare ' + name
    assert name in _lib.EXPORTS and len(_lib.EXPORTS[name][1]) == m.group(1).count(',') + 1 == 6
    assert _lib.EXPORTS[name] == _lib.EXPORTS['pe_trainer_create_models']
    assert hasattr(raw, name), 'library does not export ' + name


def test_wide_refusals_need_no_gpu():
    """by name and before any device work (this machine may have no GPU at all)"""
    stock = synth.make_weights(13, (20,))
    wide = synth.make_weights(13, (256,))
    cap = _lib.TRAIN_MAX_MODELS
    with pytest.raises(NotImplementedError, match=r'^training: units = 257 \(1\.\.256\)'):
        _lib.HipTrainer(synth.make_weights(13, (257,)), 29, 13, wide=True)
    with pytest.raises(NotImplementedError, match=r'model 2: .*units = 257'):
        _lib.HipTrainer([stock, wide, synth.make_weights(13, (257,))], 29, 13, wide=True)
    with pytest.raises(NotImplementedError, match='n_layers'):
        _lib.HipTrainer(synth.make_weights(13, (64, 64)), 29, 13, wide=True)
    with pytest.raises(NotImplementedError, match=r'model 1: .*n_layers'):
        _lib.HipTrainer([wide, synth.make_weights(13, (64, 64))], 29, 13, wide=True)
    with pytest.raises(NotImplementedError, match=r'^training: n_features = 65'):
        _lib.HipTrainer(wide, 65, 13, wide=True)
    with pytest.raises(NotImplementedError, match=r'^training: feature_size = 33'):
        _lib.HipTrainer(synth.make_weights(33, (64,)), 29, 33, wide=True)
    with pytest.raises(NotImplementedError, match='n_models = %d' % (cap + 1)):
        _lib.HipTrainer([stock] * (cap + 1), 29, 13, wide=True)
    with pytest.raises(ValueError, match='n_models'):
        _lib.HipTrainer([], 29, 13, wide=True)
    with pytest.raises(ValueError, match=r'model 1: .*takes 12 inputs, feature_size is 13'):
        _lib.HipTrainer([wide, synth.make_weights(12, (64,))], 29, 13, wide=True)


def test_wide_null_entries_are_invalid():
    lib = _lib.load()
    h = ctypes.c_void_p()
    ws = (_lib.PeWeights * 2)()                 # zeroed: null layer arrays
    ws[0].n_layers = ws[1].n_layers = 1
    assert lib.pe_trainer_create_wide(29, 13, ws, 2, 0, ctypes.byref(h)) == _lib.PE_ERR_INVALID
    assert b'model 0' in lib.pe_trainer_last_error(None) and not h.value
    assert lib.pe_trainer_create_wide(29, 13, None, 2, 0, ctypes.byref(h)) == _lib.PE_ERR_INVALID
    assert lib.pe_trainer_create_wide(29, 13, ws, 2, 0, None) == _lib.PE_ERR_INVALID


def created_or_no_device(make):
    """the object, or None where the only thing in the way is that this machine has no GPU (an EngineError from the HIP
    runtime); a refusal (NotImplementedError, ValueError) is a failure either way"""
    try:
        return make()
    except _lib.EngineError as e:
        assert e.code == _lib.PE_ERR_HIP, e
        return None


def test_parameter_count_at_256_units():
    t = created_or_no_device(lambda: _lib.HipTrainer([synth.make_weights(13, (256,)), synth.make_weights(13, (20,))], 29, 13, wide=True))
    if t is not None:
        assert t.n_params == [(13 + 256 + 1) * 3 * 256 + 256 + 1, (13 + 20 + 1) * 60 + 20 + 1]
        assert t.n_params_total == sum(t.n_params) and t.units == [256, 20]
        t.close()


def test_trainer_takes_64_units_where_the_library_runs():
    from mycroft_precise_amd.train import Trainer, TrainerGroup
    tr = created_or_no_device(lambda: Trainer(params=ModelParams(recurrent_units=64)))
    if tr is not None:
        assert tr.units == 64
        tr.close()
    group = created_or_no_device(lambda: TrainerGroup([ModelParams(recurrent_units=u) for u in (20, 64)]))
    if group is not None:
        assert group.units == [20, 64]
        group.close()
