"""The host side of the stream form of the LPC feature encoder (Part 18) and what it rests on: the definition is causal, so a
prefix of a signal encodes to a prefix of the signal's rows, bit for bit (tolerance 0: the reference evaluates frame i from samples
up to 160 i + 159 only, and every sum of a frame is the same sum in the prefix).  No GPU needed.
"""
import numpy as np
import pytest

import feature_encoder_reference as R
import feature_encoder_stream_cases as S


@pytest.fixture(scope="module")
def lpc_fn(oracle):
    from dss_amd.lpcnet_weights import synthetic_blob
    m = oracle.lpcnet_model(synthetic_blob(0))          # the chain's tables are derived, not the model's
    return lambda cep: oracle.lpc_from_cepstrum(m, np.ascontiguousarray(cep, dtype=np.float32))


@pytest.mark.parametrize("name", [n for n, _ in S.signals()])
def test_a_prefix_encodes_to_a_prefix(lpc_fn, name):
    sig = dict(S.signals())[name]
    F = len(sig) // S.FRAME
    whole = R.encode_trial(sig, lpc_fn)
    assert whole.features.shape == (F, 36)
    for k in S.prefix_lengths(F):
        part = R.encode_trial(sig[:S.FRAME * k], lpc_fn)
        assert np.array_equal(part.features, whole.features[:k]), (name, k)
        assert np.array_equal(part.scores, whole.scores[:2 * k]), (name, k)


def test_chunkings_cover_their_signals():
    for _, sig in S.signals():
        F = len(sig) // S.FRAME
        assert len(sig) == F * S.FRAME and F <= 40
        for c in S.CHUNKINGS:
            assert sum(S.chunking(c, F)) == F
    assert S.chunking("seventeen_one_fifteen", 40) == [17, 1, 15, 7]
    assert S.chunking("zero_three_zero_five", 14) == [0, 3, 0, 5, 0, 3, 0, 3]


def test_streams_check_refusals():
    from dss_amd import _lib, feature_encoder
    L = _lib.load()
    assert feature_encoder.streams_check(3, 4) == 12
    assert feature_encoder.streams_check(3, 4, [0, 4, 1]) == 5
    assert feature_encoder.streams_check(2, 0) == 0 and feature_encoder.streams_check(2, 5, [0, 0]) == 0
    for n_streams, frames_max, counts, word in ((0, 4, None, "at least 1"), (-1, 4, None, "at least 1"), (2, -1, None, "frames_max"),
                                                (2, 4, [0, 5], "stream 1"), (2, 4, [-1, 0], "stream 0"),
                                                (1, 2 ** 31 // 320 + 1, None, "too many")):
        with pytest.raises(_lib.DssError, match=word):
            feature_encoder.streams_check(n_streams, frames_max, counts)
    with pytest.raises(ValueError, match="one value per stream"):
        feature_encoder.streams_check(2, 4, [1, 2, 3])
    # NULL handles and buffers are refused with a message, no device needed
    a = np.zeros(160, np.int16)
    o = np.zeros(36, np.float32)
    seen = np.zeros(1, np.int64)
    assert L.dss_fenc_streams_push(None, a.ctypes.data, 1, None, o.ctypes.data) < 0 and L.dss_last_error()
    assert L.dss_fenc_streams_push_dev(None, a.ctypes.data, 1, None, o.ctypes.data, None) < 0
    assert L.dss_fenc_streams_reset(None, None, 0, None) < 0
    assert L.dss_fenc_streams_frames_seen(None, seen.ctypes.data) < 0
    assert L.dss_lpcnet_encoder_frames(None, a.ctypes.data, 1, o.ctypes.data) < 0
    assert L.dss_fenc_streams_create(0) is None and b"at least 1" in L.dss_last_error()
    L.dss_fenc_streams_destroy(None)


def test_encoder_opt_in_without_a_device(monkeypatch):
    from dss_amd import _lib
    L = _lib.load()
    monkeypatch.delenv("DSS_LPCNET_ENCODER", raising=False)
    assert L.lpcnet_encoder_create() is None and b"encoder" in L.dss_last_error().lower()
    monkeypatch.setenv("DSS_LPCNET_ENCODER", "0")
    assert L.lpcnet_encoder_create() is None and b"not provided" in L.dss_last_error()
    monkeypatch.setenv("DSS_LPCNET_ENCODER", "1")
    if L.dss_device_count() <= 0:
        assert L.lpcnet_encoder_create() is None
        msg = L.dss_last_error()
        assert b"encoder" in msg.lower() and b"not provided" not in msg
        import LPCNet
        with pytest.raises(MemoryError, match="encoder"):
            LPCNet.LPCFeatureEncoder()
    # the NULL-state calls are harmless either way
    assert L.lpcnet_encoder_init(None) == -1
    L.lpcnet_encoder_destroy(None)


@pytest.mark.parametrize("opt_in", [None, "1"])
def test_compute_features_is_a_failing_stub_in_both_modes(monkeypatch, opt_in):
    from dss_amd import _lib
    L = _lib.load()
    if opt_in is None:
        monkeypatch.delenv("DSS_LPCNET_ENCODER", raising=False)
    else:
        monkeypatch.setenv("DSS_LPCNET_ENCODER", opt_in)
    pcm = np.ones(4 * 160, np.int16)
    f = np.ones((4, 36), np.float32)
    assert L.lpcnet_compute_features(None, pcm.ctypes.data, f.ctypes.data) == -1 and not f.any()
    assert b"lpcnet_compute_features" in L.dss_last_error()
