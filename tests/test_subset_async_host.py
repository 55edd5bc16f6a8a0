"""CPU: the pipeline for streams that advance on their own (pe_decode_subset[_device], pe_update_subset_async) is declared,
exported and bound, refuses a null engine, and its Python wrappers refuse bad arguments before any native call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mycroft_precise_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pe_decode_subset_device', 'pe_decode_subset', 'pe_update_subset_async')


def _header():
    with open(os.path.join(REPO, 'include', 'precise_engine.h')) as f:
        return re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S))


def test_header_declares_the_three_prototypes():
    text = _header()
    for proto in (
        'int pe_decode_subset_device(pe_engine* e, const int32_t* stream_ids_dev, int32_t n_active, const float* raw_dev, '
        'double* conf_out_dev, unsigned char* fired_out_dev, void* hip_stream);',
        'int pe_decode_subset(pe_engine* e, const int32_t* stream_ids_host, int32_t n_active, const float* raw_host, '
        'double* conf_out_host, unsigned char* fired_out_host);',
        'int pe_update_subset_async(pe_engine* e, const int32_t* stream_ids_host, int32_t n_active, const int16_t* pcm_host, '
        'int32_t chunk_samples, float* raw_out_host, double* conf_out_host, unsigned char* fired_out_host);',
    ):
        assert proto in text, proto
    assert re.search(r'#define PE_ABI_VERSION 8\b', text)
    assert _lib.ABI_VERSION == 8


def test_symbols_are_exported_and_bound():
    lib = _lib.load()
    assert lib.pe_abi_version() == 8
    n_args = {'pe_decode_subset_device': 7, 'pe_decode_subset': 6, 'pe_update_subset_async': 8}
    for name in NEW:
        assert name in _lib.EXPORTS
        res, args = _lib.EXPORTS[name]
        assert res is C.c_int and len(args) == n_args[name]
        assert getattr(lib, name).argtypes == args


def test_null_engine_is_an_error_not_a_crash():
    lib = _lib.load()
    ids = np.zeros(1, np.int32)
    raw = np.zeros(1, np.float32)
    pcm = np.zeros(16, '<i2')
    assert lib.pe_decode_subset(None, ids.ctypes.data, 1, raw.ctypes.data, None, None) == _lib.PE_ERR_INVALID
    assert lib.pe_decode_subset_device(None, ids.ctypes.data, 1, raw.ctypes.data, None, None, None) == _lib.PE_ERR_INVALID
    assert lib.pe_update_subset_async(None, ids.ctypes.data, 1, pcm.ctypes.data, 16, raw.ctypes.data, None, None) == _lib.PE_ERR_INVALID


class _NoNativeCalls:
    def __getattr__(self, name):
        raise AssertionError('native call %s reached with bad arguments' % name)


def _engine(n_streams=6, n_models=1, multi=False):
    """a HipEngine shell without a device: the wrappers' own checks see n_streams / n_models, any native call fails the test"""
    e = object.__new__(_lib.HipEngine)
    e._h = C.c_void_p()
    e._lib = _NoNativeCalls()
    e._async_keep = []
    e.n_streams, e.n_models, e._multi = n_streams, n_models, multi
    return e


@pytest.mark.parametrize('multi', [False, True])
def test_update_subset_async_rejects_bad_arguments_before_any_native_call(multi):
    K = 3 if multi else 1
    e = _engine(n_models=K, multi=multi)
    ids = [4, 0, 2]
    pcm = np.zeros((3, 64), '<i2')
    ok = dict(out=np.zeros(K * 3, np.float32), conf=np.zeros(K * 3, np.float64), fired=np.zeros(K * 3, np.uint8))
    bad = {
        'out': [np.zeros(K * 3 + 1, np.float32), np.zeros(K * 3, np.float64), np.zeros((K * 3, 2), np.float32)[:, 0]],
        'conf': [np.zeros(K * 2, np.float64), np.zeros(K * 3, np.float32)],
        'fired': [np.zeros(K * 4, np.uint8), np.zeros(K * 3, bool), np.zeros(K * 3, np.int32)],
    }
    for name, arrays in bad.items():
        for a in arrays:
            with pytest.raises(ValueError, match=name):
                e.update_subset_async(ids, pcm, **dict(ok, **{name: a}))
    for wrong in ([0, 6], [-1, 2], [6]):
        with pytest.raises(ValueError, match='0..5'):
            e.update_subset_async(wrong, pcm[:len(wrong)], **ok)
    with pytest.raises(ValueError, match='twice'):
        e.update_subset_async([1, 3, 1], pcm, **ok)
    for rows in (2, 4):
        with pytest.raises(ValueError, match='3 active streams'):
            e.update_subset_async(ids, np.zeros((rows, 64), '<i2'), **ok)
    with pytest.raises(ValueError, match='6 active streams'):           # ids None: every stream
        e.update_subset_async(None, pcm)
    # (and a good call does reach the library)
    with pytest.raises(AssertionError, match='pe_update_subset_async'):
        e.update_subset_async(ids, pcm, **ok)


def test_decode_subset_rejects_bad_arguments_before_any_native_call():
    e = _engine(n_models=2, multi=True)
    for wrong in ([0, 6], [-1]):
        with pytest.raises(ValueError, match='0..5'):
            e.decode_subset(wrong, np.zeros(2 * len(wrong), np.float32))
    with pytest.raises(ValueError, match='twice'):
        e.decode_subset([5, 5], np.zeros(4, np.float32))
    with pytest.raises(ValueError, match='4 raw outputs'):
        e.decode_subset([1, 2], np.zeros(2, np.float32))
    with pytest.raises(AssertionError, match='pe_decode_subset'):
        e.decode_subset([1, 2], np.zeros(4, np.float32))


def test_listener_subset_calls_check_ids_and_rows_first():
    from mycroft_precise_amd.network_runner import BatchedListener
    ls = object.__new__(BatchedListener)
    ls.n_streams, ls._trigger, ls.engine = 6, True, _engine()
    pcm = np.zeros((2, 64), '<i2')
    for call in (ls.update_raw_async, ls.update_detect, ls.update_detect_async):
        kw = {'streams': [0, 6]}
        with pytest.raises(ValueError):
            call(pcm, **kw)
        with pytest.raises(ValueError):
            call(pcm, streams=[3, 3])
        with pytest.raises(ValueError):
            call(pcm, streams=[0, 1, 2])
        with pytest.raises(EOFError):
            call(np.zeros((2, 0), '<i2'), streams=[0, 1])
