"""CPU: the surface of the batched clip path (pe_vectorize_clips / pe_score_clips) that needs no device -- the ABI table,
the header, and the argument errors that are raised before the library is even loaded."""
import os
import re

import numpy as np
import pytest

from conftest import REPO
from mycroft_precise_amd import _lib
from mycroft_precise_amd import params as P
from mycroft_precise_amd.util import InvalidAudio

NEW = ('pe_vectorize_clips', 'pe_score_clips', 'pe_set_clip_pass_bytes')


def test_new_entry_points_are_declared_and_bound():
    text = open(os.path.join(REPO, 'include', 'precise_engine.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(pe_[a-z_0-9]+)\s*\(', text))          # (the expression of test_abi.py)
    for name in NEW:
        assert name in _lib.EXPORTS and name in declared
    assert sorted(_lib.EXPORTS) == sorted(declared)
    assert _lib.ABI_VERSION == 8 and re.search(r'#define\s+PE_ABI_VERSION\s+8\b', text)
    # arity: handle + the arguments of the header
    assert len(_lib.EXPORTS['pe_vectorize_clips'][1]) == 8
    assert len(_lib.EXPORTS['pe_score_clips'][1]) == 7
    assert len(_lib.EXPORTS['pe_set_clip_pass_bytes'][1]) == 2
    for name in ('vectorize_clips', 'score_clips', 'set_clip_pass_bytes'):
        assert callable(getattr(_lib.HipEngine, name))


@pytest.fixture()
def no_library(monkeypatch):
    """any attempt to load the library (or to create an engine) fails the test"""
    def boom(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', boom)
    monkeypatch.setattr(_lib.HipEngine, '__init__', boom)


def test_empty_clip_is_invalid_audio_before_any_device_work(no_library):
    from mycroft_precise_amd import vectorization as V
    from mycroft_precise_amd.network_runner import HipRunner
    with pytest.raises(InvalidAudio):
        V.vectorize_batch([np.zeros(0)])
    with pytest.raises(InvalidAudio):
        V.vectorize_batch([np.ones(4000), np.zeros(0, np.float32), np.ones(10)])
    runner = HipRunner.__new__(HipRunner)             # (no engine behind it: predict_clips must not get that far)
    with pytest.raises(InvalidAudio):
        runner.predict_clips([np.ones(4000), np.zeros(0)])


def test_no_clips_give_an_empty_batch(no_library):
    from mycroft_precise_amd import vectorization as V
    out = V.vectorize_batch([])
    assert out.shape == (0, P.pr.n_features, P.pr.feature_size) == (0, 29, 13)
    saved = dict(P.pr.__dict__)
    try:
        P.pr.__dict__['use_delta'] = True
        assert V.vectorize_batch([]).shape == (0, 29, 26)
        P.pr.__dict__.update(use_delta=False, vectorizer=P.Vectorizer.mels)
        assert V.vectorize_batch([]).shape == (0, 29, 20)
    finally:
        P.pr.__dict__.clear()
        P.pr.__dict__.update(saved)


def test_clips_are_concatenated_once_in_the_narrowest_common_format():
    clips = [np.arange(5, dtype=np.float32), np.arange(3, dtype=np.float32)]
    audio, offsets, fmt = _lib.HipEngine._clips(clips)
    assert fmt == 1 and audio.dtype == np.float32 and offsets.tolist() == [0, 5, 8] and offsets.dtype == np.int64
    assert np.array_equal(audio, np.concatenate(clips))
    audio, offsets, fmt = _lib.HipEngine._clips([clips[0], np.arange(3, dtype=np.float64)])
    assert fmt == 0 and audio.dtype == np.float64 and offsets.tolist() == [0, 5, 8]
    audio, offsets, fmt = _lib.HipEngine._clips([])
    assert fmt == 0 and audio.size == 0 and offsets.tolist() == [0]
    with pytest.raises(ValueError):
        _lib.HipEngine._clips([np.zeros((2, 3))])
