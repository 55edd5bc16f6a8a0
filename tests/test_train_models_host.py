"""CPU: the C ABI declares the several-network trainer, its refusals happen before any device work and name what they
refuse, and ``TrainerGroup`` checks its arguments before it touches the library's GPU side."""
import ctypes
import os
import re

import pytest

from conftest import REPO
from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd.model import ModelParams

NEW_SYMBOLS = ('pe_trainer_create_models', 'pe_trainer_n_models', 'pe_trainer_n_params_model', 'pe_trainer_step_models',
               'pe_trainer_set_validation', 'pe_trainer_n_samples', 'pe_trainer_evaluate_models')


def test_models_abi_is_declared_and_bound():
    text = open(os.path.join(REPO, 'include', 'precise_engine.h')).read()
    assert re.search(r'#define\s+PE_ABI_VERSION\s+8\b', text) and _lib.ABI_VERSION == 8
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r'\b%s\s*\(([^)]*)\)' % name, code)
        assert m, 'the header does not declare ' + name
        n_args = 0 if m.group(1).strip() in ('', 'void') else m.group(1).count(',') + 1
        assert name in _lib.EXPORTS, name
        assert len(_lib.EXPORTS[name][1]) == n_args, name
        assert hasattr(raw, name), 'library does not export ' + name
    cap = re.search(r'#define\s+PE_TRAIN_MAX_MODELS\s+(\d+)', code)
    assert cap and int(cap.group(1)) == _lib.TRAIN_MAX_MODELS >= 16
    for name, value in (('HOST', _lib.TRAIN_SOURCE_HOST), ('DATA', _lib.TRAIN_SOURCE_DATA), ('VALIDATION', _lib.TRAIN_SOURCE_VALIDATION)):
        assert re.search(r'#define\s+PE_TRAIN_SOURCE_%s\s+%d\b' % (name, value), code)
    # pe_train_hparams: the header's fields in the binding's order, and the size the C compiler gives them
    body = re.search(r'typedef\s+struct\s+pe_train_hparams\s*\{(.*?)\}\s*pe_train_hparams\s*;', code, flags=re.S)
    assert body
    fields = [f.strip() for decl in body.group(1).split(';') if decl.strip() for f in decl.strip().split(None, 1)[1].split(',')]
    assert fields == [f[0] for f in _lib.PeTrainHparams._fields_]
    assert ctypes.sizeof(_lib.PeTrainHparams) == 40


def test_create_models_refusals_need_no_gpu():
    """by name and before any device work (this machine may have no GPU at all)"""
    stock = synth.make_weights(13, (20,))
    cap = _lib.TRAIN_MAX_MODELS
    with pytest.raises(ValueError, match='n_models'):
        _lib.HipTrainer([], 29, 13)
    with pytest.raises(NotImplementedError, match='n_models = %d' % (cap + 1)):
        _lib.HipTrainer([stock] * (cap + 1), 29, 13)
    with pytest.raises(NotImplementedError, match=r'model 2: .*units = 33'):
        _lib.HipTrainer([stock, stock, synth.make_weights(13, (33,)), stock], 29, 13)
    with pytest.raises(NotImplementedError, match=r'model 1: .*n_layers'):
        _lib.HipTrainer([stock, synth.make_weights(13, (20, 20))], 29, 13)
    with pytest.raises(ValueError, match=r'model 1: .*takes 12 inputs, feature_size is 13'):
        _lib.HipTrainer([stock, synth.make_weights(12, (20,))], 29, 13)
    # the shared fields carry no model index, and a list of one reads like the single trainer
    with pytest.raises(NotImplementedError, match=r'^training: n_features = 65'):
        _lib.HipTrainer([stock, stock], 65, 13)
    with pytest.raises(NotImplementedError, match=r'^training: units = 33'):
        _lib.HipTrainer([synth.make_weights(13, (33,))], 29, 13)


def test_null_entries_are_invalid():
    lib = _lib.load()
    h = ctypes.c_void_p()
    ws = (_lib.PeWeights * 2)()                 # zeroed: n_layers 0, null arrays
    ws[0].n_layers = ws[1].n_layers = 1
    assert lib.pe_trainer_create_models(29, 13, ws, 2, 0, ctypes.byref(h)) == _lib.PE_ERR_INVALID
    assert b'model 0' in lib.pe_trainer_last_error(None) and not h.value
    assert lib.pe_trainer_create_models(29, 13, None, 2, 0, ctypes.byref(h)) == _lib.PE_ERR_INVALID
    assert lib.pe_trainer_create_models(29, 13, ws, 2, 0, None) == _lib.PE_ERR_INVALID
    assert lib.pe_trainer_n_models(None) == -1 and lib.pe_trainer_n_params_model(None, 0) == -1
    assert lib.pe_trainer_n_samples(None, _lib.TRAIN_SOURCE_DATA) == -1


def test_trainer_group_argument_errors():
    from mycroft_precise_amd.train import TrainerGroup
    two = [ModelParams(recurrent_units=8), ModelParams(recurrent_units=20)]
    with pytest.raises(ValueError, match='at least one candidate'):
        TrainerGroup([])
    with pytest.raises(ValueError, match='3 seeds for 2 candidates'):
        TrainerGroup(two, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match='1 weights for 2 candidates'):
        TrainerGroup(two, weights=[None])
