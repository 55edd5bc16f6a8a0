"""CPU: the float32 wide / stacked engine (33..256 units, one or two layers) takes up to 32 inputs per frame -- use_delta over
<= 16 coefficients, or 17..32 coefficients -- so pe_create no longer refuses what the trainers save.  What it
still refuses, it refuses by name and before any device work: this machine may have no GPU at all."""
import pytest

from mycroft_precise_amd import _lib, synth
from mycroft_precise_amd import params as P


def created_or_no_device(make):
    """the object, or None where the only thing in the way is that this machine has no GPU (an EngineError from the HIP
    runtime); a refusal (NotImplementedError, ValueError) is a failure either way"""
    try:
        return make()
    except _lib.EngineError as e:
        assert e.code == _lib.PE_ERR_HIP, e
        return None


def params(**kw):
    hpr = P.pr.copy()
    hpr.__dict__.update(kw)
    return hpr


DELTA = dict(use_delta=True)
COEF20 = dict(n_fft=1024, n_filt=40, n_mfcc=20)


@pytest.mark.parametrize('kw,n_in,units', [(DELTA, 26, (64,)), (DELTA, 26, (40, 33)), (COEF20, 20, (72, 200))],
                         ids=['delta-64', 'delta-40x33', 'coef20-72x200'])
def test_wide_engines_with_two_input_groups_are_created(kw, n_in, units):
    hpr = params(**kw)
    assert hpr.feature_size == n_in
    eng = created_or_no_device(lambda: _lib.HipEngine(hpr, synth.make_weights(n_in=n_in, units=units, seed=41)))
    if eng is not None:
        assert eng.feature_size == n_in and eng.units == units[-1]
        eng.close()


def test_refusals_need_no_gpu():
    with pytest.raises(NotImplementedError, match=r'use_delta over more than 16 coefficients \(n_mfcc = 17: 34 inputs'):
        _lib.HipEngine(params(use_delta=True, n_fft=1024, n_filt=40, n_mfcc=17), synth.make_weights(n_in=34, units=(64,), seed=41))
    with pytest.raises(NotImplementedError, match='use_delta has no bf16-operand wide-GRU kernel'):
        _lib.HipEngine(params(**DELTA), synth.make_weights(n_in=26, units=(64,), seed=41), gru_precision='bf16')
    with pytest.raises(NotImplementedError, match=r'more than 16 coefficients per frame \(n_mfcc = 20\) have no bf16-operand wide-GRU kernel'):
        _lib.HipEngine(params(**COEF20), synth.make_weights(n_in=20, units=(72, 200), seed=41), gru_precision='bf16')
    # the limits that were there before: layers, widths, bf16 rows
    with pytest.raises(NotImplementedError, match='256 units'):
        _lib.HipEngine(params(**DELTA), synth.make_weights(n_in=26, units=(257,), seed=41))
    with pytest.raises(NotImplementedError, match='ring_precision'):
        _lib.HipEngine(params(), synth.make_weights(units=(64,), seed=41), gru_precision='bf16', ring_precision='bf16')
