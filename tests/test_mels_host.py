"""CPU: models trained on Vectorizer.mels features -- the reference the GPU tests use pinned to the reference's
own fixture, the limits refused by name before any device work, and the shape bookkeeping of HipEngine / Listener with rows
``n_filt`` wide.  This machine may have no GPU at all."""
import json

import numpy as np
import pytest

import mels_reference as M
from conftest import golden
from mycroft_precise_amd import _lib, model, synth
from mycroft_precise_amd import params as P
from mycroft_precise_amd import vectorization as V


def params(**kw):
    hpr = P.pr.copy()
    hpr.__dict__.update(vectorizer=P.Vectorizer.mels)
    hpr.__dict__.update(kw)
    return hpr


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_reference_is_pinned_to_the_reference_fixture():
    """tests/golden/vectorize_mels.npz: the reference's own vectorize / vectorize_raw under pr.vectorizer = mels"""
    g = golden('vectorize_mels.npz')
    pr = M.params()
    assert pr.feature_size == pr.n_filt == 20 and M.row_width(pr) == 20
    for name in ('short', 'long', 'one_window', 'zeros'):
        assert np.array_equal(M.vectorize_raw(g['audio_' + name], pr), g['raw_' + name]), name
    for name in ('short', 'long', 'one_window'):
        assert np.array_equal(M.vectorize(g['audio_' + name], pr), g['vec_' + name]), name
    assert np.all(g['raw_zeros'] == np.log(np.finfo(float).eps))
    assert M.params(use_delta=True).feature_size == 40


def test_reference_listeners_agree_and_keep_filter_zero():
    """the batched restatement is the single-stream one per stream; coefficient 0 is filter 0, not the log power"""
    pr = M.params()
    w = synth.make_weights(n_in=20, units=(20,), seed=1)
    pcm = synth.batch_pcm(2, 6, 1023)
    one = [M.MelsListener(w, pr) for _ in range(2)]
    many = M.BatchedMels(w, 2, pr)
    for u in range(6):
        got = many.update_raw(pcm[u])
        want = [r.update_raw32(pcm[u, j].tobytes()) for j, r in enumerate(one)]
        # (one BLAS call over both streams and one per stream may round the last bit differently)
        assert np.allclose(got, np.array(want, dtype=np.float32), rtol=0, atol=1e-6), u
    assert many.mfccs.shape == (2, pr.n_features, 20)
    assert np.allclose(many.mfccs[1], one[1].mfccs, rtol=1e-13, atol=0)
    audio = pcm[:, 0].reshape(-1).astype(np.float32) / np.float32(32768.0)
    rows = M.vectorize_raw(audio, pr)
    mf = M.ol.vectorize_raw(audio, M.ol.Params())
    assert not np.allclose(rows[:, 0], mf[:, 0])                  # sonopy Q7 belongs to mfcc_spec only


# ---- refusals: each by name, none needs a device ------------------------------------------------------------------------
def w_in(n_in, units=(20,)):
    return synth.make_weights(n_in=n_in, units=units, seed=1)


def test_refusals_need_no_gpu(stock_weights):
    with pytest.raises(NotImplementedError, match=r'Vectorizer.mels feeds 20 inputs per frame, this network takes 13'):
        _lib.HipEngine(params(), stock_weights)
    with pytest.raises(NotImplementedError, match=r'Vectorizer.mels feeds 32 inputs per frame, this network takes 16'):
        _lib.HipEngine(params(n_filt=16, use_delta=True), w_in(16))
    with pytest.raises(NotImplementedError, match=r'n_filt = 40 values per frame: the networks take up to 32 inputs'):
        _lib.HipEngine(params(n_filt=40), w_in(40))
    with pytest.raises(NotImplementedError, match=r'n_filt = 20: rows of more than 16 values feed a float32 network without'):
        _lib.HipEngine(params(use_delta=True), w_in(40))
    with pytest.raises(NotImplementedError, match=r'n_filt = 20: rows of more than 16 values feed a float32 network without'):
        _lib.HipEngine(params(), w_in(20), gru_precision='bf16')
    with pytest.raises(NotImplementedError, match=r'n_filt = 20: rows of more than 16 values feed a float32 network without'):
        _lib.HipEngine(params(), w_in(20, (64,)), gru_precision='bf16', ring_precision='bf16')
    bank = V.speechpy_filterbank(16000, 20, 257)
    with pytest.raises(NotImplementedError, match=r'the speechpy filterbank belongs to Vectorizer.speechpy_mfccs'):
        _lib.HipEngine(params(), w_in(20), mel_filters=bank)
    # a two-model engine: every model is checked
    with pytest.raises(NotImplementedError, match=r'feeds 20 inputs per frame, this network takes 13'):
        _lib.HipEngine(params(), [w_in(20), stock_weights])


def test_listeners_refuse_before_the_library_is_touched(stock_weights, monkeypatch):
    from mycroft_precise_amd.network_runner import BatchedListener, MultiModelListener, _require_streamable

    def no_library():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', no_library)
    with pytest.raises(NotImplementedError, match=r'feeds 20 inputs per frame, this network takes 13'):
        BatchedListener(stock_weights, 4, params=params())
    with pytest.raises(NotImplementedError, match=r'n_filt = 40 values per frame'):
        BatchedListener(w_in(40), 4, params=params(n_filt=40))
    with pytest.raises(NotImplementedError, match=r'feeds 20 inputs per frame, this network takes 13'):
        MultiModelListener([stock_weights], 4, params=params())
    _require_streamable(params())                                  # mels within the limits: accepted
    _require_streamable(params(n_filt=32))
    with pytest.raises(NotImplementedError):
        _require_streamable(params(vectorizer=7))


# ---- shape bookkeeping: a stand-in library that accepts every call ---------------------------------------------------------
class _AnyCall:
    """every pe_* entry point: returns PE_OK, touches nothing"""
    def __init__(self):
        self.created = []

    def __getattr__(self, name):
        def call(*args):
            if name in ('pe_create', 'pe_create_models'):
                self.created.append(args[0]._obj)                  # the PeParams handed over
                args[-1]._obj.value = 1                            # a non-null handle
            return _lib.PE_OK
        return call


@pytest.fixture
def any_library(monkeypatch):
    lib = _AnyCall()
    monkeypatch.setattr(_lib, 'load', lambda: lib)
    return lib


@pytest.fixture
def restore_pr():
    saved = dict(P.pr.__dict__)
    yield
    P.pr.__dict__.clear()
    P.pr.__dict__.update(saved)


def test_engine_passes_the_vectorizer_and_sizes_rows_from_n_filt(any_library):
    eng = _lib.HipEngine(params(n_filt=24, n_fft=1024), w_in(24), n_streams=3)
    assert any_library.created[0].vectorizer == 1 and any_library.created[0].n_filt == 24
    assert eng.mels and eng.row_width == 24 and eng.feature_size == 24 and eng.n_mfcc == 13
    assert eng.get_vectors().shape == (3, eng.n_features, 24)
    assert eng.update_vectors(np.zeros((3, 1024), np.int16)).shape == (3, eng.n_features, 24)
    eng.set_vectors(np.zeros((3, eng.n_features, 24), np.float32))
    with pytest.raises(ValueError, match=r'expected \[3, \d+, 24\]'):
        eng.set_vectors(np.zeros((3, eng.n_features, 13), np.float32))
    assert eng.predict(np.zeros((2, eng.n_features, 24), np.float32)).shape == (2, 1)
    with pytest.raises(ValueError):
        eng.predict(np.zeros((2, eng.n_features, 13), np.float32))
    clips = [np.zeros(4000), np.zeros(30000)]
    assert eng.vectorize_clips(clips, 24000).shape == (2, eng.n_features, 24)
    assert eng.vectorize_clips(clips, 24000, mels=True).shape == (2, eng.n_features, 24)
    eng._h.value = 0
    d = _lib.HipEngine(params(n_filt=16, use_delta=True), w_in(32))
    assert d.row_width == 16 and d.feature_size == 32
    d._h.value = 0
    # an mfccs engine is sized as before
    m = _lib.HipEngine(P.pr.copy(), w_in(13))
    assert any_library.created[-1].vectorizer == 2
    assert not m.mels and m.row_width == 13 and m.feature_size == 13
    assert m.vectorize_clips(clips, 24000, mels=True).shape == (2, m.n_features, 20)
    m._h.value = 0


def test_listener_window_is_n_filt_wide_from_a_params_file(any_library, restore_pr, tmp_path):
    from mycroft_precise_amd.network_runner import Listener
    name = str(tmp_path / 'mels.npz')
    model.save_weights(name, w_in(20))
    with open(name + '.params', 'w') as f:
        json.dump(dict(P.pr.__dict__, vectorizer=P.Vectorizer.mels), f)
    lis = Listener(name)
    assert lis.pr.vectorizer == P.Vectorizer.mels and lis.pr.feature_size == 20
    assert lis.runner.engine.row_width == 20 and any_library.created[0].vectorizer == 1
    assert lis.mfccs.shape == (lis.pr.n_features, 20)
    window = np.arange(lis.pr.n_features * 20, dtype=np.float64).reshape(-1, 20)
    lis.mfccs = window
    assert np.array_equal(lis.mfccs, window)
    with pytest.raises(ValueError):
        lis.mfccs = np.zeros((lis.pr.n_features, 13))
    lis.runner.engine._h.value = 0
