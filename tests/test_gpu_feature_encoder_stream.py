"""The stream form of the LPC feature encoder (Part 18, csrc/feature_encoder_stream.hip) against the trial-list form (Part 16):
the method is causal and the two forms share their arithmetic term for term (csrc/fenc_blocks.h), so every comparison here is
``array_equal`` on all 36 columns against ``LpcFeatureEncoderGPU.features_trials(signal, [0, n], total=True)``, whatever the
chunking.  Signals and chunkings: tests/feature_encoder_stream_cases.py.
"""
import os
import subprocess
import sys
import sysconfig

import numpy as np
import pytest

import feature_encoder_reference as R
import feature_encoder_stream_cases as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNALS = S.signals()
FRAME = S.FRAME
JUNK = 12345            # what the audio rows past a stream's count hold: never read


@pytest.fixture(scope="module")
def whole():
    """name -> float32 (F, 36): every signal as one trial through the trial-list form, once."""
    from dss_amd.feature_encoder import LpcFeatureEncoderGPU
    e = LpcFeatureEncoderGPU()
    out = {name: e.features_trials(sig, [0, len(sig)], total=True)[0] for name, sig in SIGNALS}
    e.trial = lambda sig: e.features_trials(np.ascontiguousarray(sig), [0, len(sig)], total=True)[0]
    out["_enc"] = e
    yield out
    e.close()


@pytest.fixture(scope="module")
def one():
    from dss_amd.feature_encoder import LpcFeatureStreamsGPU
    s = LpcFeatureStreamsGPU(1)
    yield s
    s.close()


def _push_chunks(streams, sig, chunks):
    """One stream: the signal in pushes of `chunks` frames; a 0 is a push the stream sits out (counts = [0] beside junk audio)."""
    rows, at = [], 0
    for c in chunks:
        if c == 0:
            out = streams.push(np.full((1, 2 * FRAME), JUNK, np.int16), counts=[0], total=True)
            assert out.shape == (1, 2, 36) and not out.any()
            continue
        out = streams.push(sig[None, at:at + c * FRAME], total=True)
        assert out.shape == (1, c, 36) and out.dtype == np.float32
        rows.append(out[0])
        at += c * FRAME
    assert at == len(sig)
    return np.concatenate(rows)


@pytest.mark.parametrize("chunks", S.CHUNKINGS)
@pytest.mark.parametrize("name", [n for n, _ in SIGNALS])
def test_any_chunking_gives_the_bits_of_the_whole_trial(whole, one, name, chunks):
    sig = dict(SIGNALS)[name]
    F = len(sig) // FRAME
    one.reset()
    got = _push_chunks(one, sig, S.chunking(chunks, F))
    assert np.isfinite(got).all() and np.array_equal(got, whole[name]), (name, chunks)
    assert one.frames_seen.tolist() == [F]


def test_streams_on_their_own_schedules(whole):
    from dss_amd.feature_encoder import LpcFeatureStreamsGPU
    plans = [S.chunking(c, len(sig) // FRAME) for (_, sig), c in
             zip(SIGNALS, ("fours", "zero_three_zero_five", "ones", "seventeen_one_fifteen", "sixteens"))]
    sigs = [sig for _, sig in SIGNALS]
    st = LpcFeatureStreamsGPU(len(sigs))
    try:
        rows = [[] for _ in sigs]
        at = [0] * len(sigs)
        for r in range(max(len(p) for p in plans)):
            counts = [p[r] if r < len(p) else 0 for p in plans]
            K = max(counts)
            if K == 0:
                continue
            audio = np.full((len(sigs), K * FRAME), JUNK, np.int16)
            for s, c in enumerate(counts):
                audio[s, :c * FRAME] = sigs[s][at[s]:at[s] + c * FRAME]
            out = st.push(audio, counts=counts, total=True)
            assert out.shape == (len(sigs), K, 36)
            for s, c in enumerate(counts):
                rows[s].append(out[s, :c])
                assert not out[s, c:].any(), (r, s)                 # rows past the count are zeros
                at[s] += c * FRAME
            assert st.frames_seen.tolist() == [a // FRAME for a in at]
        for s, (name, sig) in enumerate(SIGNALS):
            assert at[s] == len(sig)
            assert np.array_equal(np.concatenate(rows[s]), whole[name]), name
        out20 = st.push(np.zeros((len(sigs), FRAME), np.int16))
        assert out20.shape == (len(sigs), 1, 20)
    finally:
        st.close()


def test_reset_of_one_stream_and_of_all(whole):
    from dss_amd.feature_encoder import LpcFeatureStreamsGPU
    names = ("forty", "white35", "zeros_then_speech")
    sigs = [dict(SIGNALS)[n][:14 * FRAME] for n in names]
    audio = np.stack(sigs)
    cut = 5 * FRAME
    st = LpcFeatureStreamsGPU(3)
    fresh = LpcFeatureStreamsGPU(3)
    try:
        first = st.push(audio[:, :cut], total=True)
        st.reset([1])
        assert st.frames_seen.tolist() == [5, 0, 5]
        rest = st.push(audio[:, cut:], total=True)
        assert st.frames_seen.tolist() == [14, 9, 14]
        for s in (0, 2):                                            # the others are unaffected
            assert np.array_equal(np.concatenate([first[s], rest[s]]), whole[names[s]][:14])
        assert np.array_equal(first[1], whole[names[1]][:5])
        assert np.array_equal(rest[1], whole["_enc"].trial(sigs[1][cut:]))      # a fresh trial on the rest of its audio
        st.reset()
        assert st.frames_seen.tolist() == [0, 0, 0]
        again = st.push(audio, total=True)
        new = fresh.push(audio, total=True)
        assert np.array_equal(again, new)                           # a new handle gives the bits of a reset one
        for s in range(3):
            assert np.array_equal(again[s], whole[names[s]][:14])
    finally:
        st.close()
        fresh.close()


def test_host_and_device_entry_points_give_the_same_bits(whole):
    import torch
    from dss_amd.feature_encoder import LpcFeatureStreamsGPU
    names = ("forty", "white35")
    audio = np.stack([dict(SIGNALS)[n][:35 * FRAME] for n in names])
    counts = [[4, 3], [17, 0], [14, 32]]
    st = LpcFeatureStreamsGPU(2)
    try:
        host, at = [], [0, 0]
        for c in counts:
            K = max(c)
            a = np.full((2, K * FRAME), JUNK, np.int16)
            for s in range(2):
                a[s, :c[s] * FRAME] = audio[s, at[s]:at[s] + c[s] * FRAME]
                at[s] += c[s] * FRAME
            host.append((a, st.push(a, counts=c, total=True)))
        # the same pushes on device buffers, on the current stream ...
        st.reset()
        for (a, want), c in zip(host, counts):
            out = st.push_torch(torch.from_numpy(a).cuda(), counts=c, total=True)
            assert out.is_cuda and out.dtype == torch.float32 and np.array_equal(out.cpu().numpy(), want)
        # ... and on a side stream, reset included: complete after that stream's synchronisation
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        d_in = [torch.from_numpy(a).cuda() for a, _ in host]
        torch.cuda.synchronize()
        st.reset(stream=side.cuda_stream)
        outs = [st.push_torch(d, counts=c, total=True, stream=side.cuda_stream) for d, c in zip(d_in, counts)]
        out20 = st.push_torch(d_in[0], stream=side.cuda_stream)
        side.synchronize()
        for out, (_, want) in zip(outs, host):
            assert np.array_equal(out.cpu().numpy(), want)
        assert out20.shape == (2, 4, 20)
        assert st.frames_seen.tolist() == [39, 39]
        got = [np.concatenate([w[s, :c[s]] for (_, w), c in zip(host, counts)]) for s in range(2)]
        for s in range(2):
            assert np.array_equal(got[s], whole[names[s]][:35])
    finally:
        st.close()


def test_all_zero_stream_is_the_references_own_numbers(oracle, one):
    from dss_amd.lpcnet_weights import synthetic_blob
    m = oracle.lpcnet_model(synthetic_blob(0))
    sig = dict(SIGNALS)["zeros"]
    own = R.encode_trial(sig, lambda cep: oracle.lpc_from_cepstrum(m, np.ascontiguousarray(cep, dtype=np.float32)))
    for chunks in ("ones", "whole"):
        one.reset()
        got = _push_chunks(one, sig, S.chunking(chunks, len(sig) // FRAME))
        assert np.array_equal(got, own.features)          # cepstrum included: equal inputs, equal order, equal bits


def _xiph_loop(L, st, sig):
    out = np.zeros((len(sig) // FRAME, 36), np.float32)
    for i in range(len(out)):
        frame = np.ascontiguousarray(sig[i * FRAME:(i + 1) * FRAME])
        assert L.lpcnet_compute_single_frame_features(st, frame.ctypes.data, out[i].ctypes.data) == 0
    return out


def test_xiph_encoder_symbols_with_the_opt_in(whole, monkeypatch):
    from dss_amd import _lib
    L = _lib.load()
    sig = dict(SIGNALS)["zeros_then_speech"]
    monkeypatch.setenv("DSS_LPCNET_ENCODER", "1")
    st = L.lpcnet_encoder_create()
    assert st, L.dss_last_error()
    try:
        monkeypatch.delenv("DSS_LPCNET_ENCODER")                       # read at create only: the state stays bound
        assert L.lpcnet_encoder_create() is None and b"encoder" in L.dss_last_error().lower()
        loop = _xiph_loop(L, st, sig)
        assert np.array_equal(loop, whole["zeros_then_speech"])       # a 160-sample loop equals the whole trial
        assert L.lpcnet_encoder_init(st) == 0                          # init resets
        assert np.array_equal(_xiph_loop(L, st, sig[:3 * FRAME]), whole["zeros_then_speech"][:3])
        assert L.lpcnet_encoder_init(st) == 0
        out = np.zeros((len(sig) // FRAME, 36), np.float32)
        assert L.dss_lpcnet_encoder_frames(st, sig.ctypes.data, len(out), out.ctypes.data) == len(out)
        assert np.array_equal(out, loop)
        assert L.dss_lpcnet_encoder_frames(st, None, 0, None) == 0
        # failures: -1, zeros, counted; the four-frame packet form is a stub on a live state too
        before = L.dss_error_count()
        f36 = np.ones(36, np.float32)
        assert L.lpcnet_compute_single_frame_features(st, None, f36.ctypes.data) == -1 and not f36.any()
        assert L.dss_error_count() == before + 1
        f4 = np.ones((4, 36), np.float32)
        assert L.lpcnet_compute_features(st, sig.ctypes.data, f4.ctypes.data) == -1 and not f4.any()
    finally:
        L.lpcnet_encoder_destroy(st)


def test_drop_in_feature_encoder(whole, monkeypatch):
    import LPCNet
    sig = dict(SIGNALS)["forty"]
    want = whole["forty"][:, :20]
    monkeypatch.delenv("DSS_LPCNET_ENCODER", raising=False)
    with pytest.raises(MemoryError, match="encoder"):
        LPCNet.LPCFeatureEncoder()
    monkeypatch.setenv("DSS_LPCNET_ENCODER", "1")
    enc = LPCNet.LPCFeatureEncoder()
    a = enc.compute_LPC_features(sig[:13 * FRAME + 77])               # the 77 samples behind the last whole frame are dropped
    assert a.dtype == np.float32 and a.shape == (13, 20)
    b = enc.compute_LPC_features(sig[13 * FRAME:])
    assert np.array_equal(np.concatenate([a, b]), want)               # two calls equal one call on the concatenation
    enc.reset_encoder()
    assert np.array_equal(enc.compute_LPC_features(sig), want)
    assert enc.compute_LPC_features(np.zeros(159, np.int16)).shape == (0, 20)
    with pytest.raises(TypeError, match="incorrect type"):
        enc.compute_LPC_features([0] * 160)
    with pytest.raises(ValueError, match="wrong number of dimensions"):
        enc.compute_LPC_features(np.zeros((2, 160), np.int16))
    with pytest.raises(ValueError, match="dtype mismatch"):
        enc.compute_LPC_features(np.zeros(160, np.float32))
    del enc


def _ref_lpcnet_module():
    return os.path.join(ROOT, "oracle", "_ref", "LPCNet" + sysconfig.get_config_var("EXT_SUFFIX"))


@pytest.mark.skipif(not os.path.exists(_ref_lpcnet_module()),
                    reason="oracle/_ref/LPCNet module not built (build() compiles it where the reference tree is present)")
def test_the_references_own_wrapper_in_a_child_process(whole, tmp_path):
    """The reference's Cython LPCFeatureEncoder, linked to the library unchanged, in a fresh process with the opt-in: its
    160-sample loop over lpcnet_compute_single_frame_features gives the trial-list bits, and its state carries across calls."""
    sig = dict(SIGNALS)["zeros_then_speech"]
    np.save(tmp_path / "sig.npy", sig)
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import LPCNet as M\n"
        "assert M.__file__.endswith(%r), M.__file__\n"
        "sig = np.load(%r)\n"
        "e = M.LPCFeatureEncoder()\n"
        "one = e.compute_LPC_features(sig)\n"
        "e.reset_encoder()\n"
        "two = np.concatenate([e.compute_LPC_features(sig[:800]), e.compute_LPC_features(sig[800:])])\n"
        "np.save(%r, np.stack([one, two]))\n"
        % (os.path.dirname(_ref_lpcnet_module()), os.sep + "LPCNet" + sysconfig.get_config_var("EXT_SUFFIX"),
           str(tmp_path / "sig.npy"), str(tmp_path / "out.npy")))
    env = {k: v for k, v in os.environ.items() if k not in ("DSS_LPCNET_WEIGHTS", "PYTHONPATH")}
    env["DSS_LPCNET_ENCODER"] = "1"
    subprocess.check_call([sys.executable, "-c", code], env=env)
    one, two = np.load(tmp_path / "out.npy")
    want = whole["zeros_then_speech"][:, :20]
    assert one.dtype == np.float32 and np.array_equal(one, want)
    assert np.array_equal(two, want)


def test_refusals_leave_the_handle_working(whole):
    import torch
    from dss_amd import _lib
    from dss_amd.feature_encoder import LpcFeatureStreamsGPU
    with pytest.raises(_lib.DssError, match="at least 1"):
        LpcFeatureStreamsGPU(0)
    sig = dict(SIGNALS)["square"]
    st = LpcFeatureStreamsGPU(2)
    try:
        half = st.push(np.stack([sig[:4 * FRAME]] * 2), total=True)
        with pytest.raises(ValueError, match="int16"):
            st.push(np.zeros((2, 160), np.float32))
        with pytest.raises(ValueError, match="two-dimensional"):
            st.push(np.zeros(320, np.int16))
        with pytest.raises(ValueError, match="n_streams, 160 k"):
            st.push(np.zeros((2, 161), np.int16))
        with pytest.raises(ValueError, match="n_streams, 160 k"):
            st.push(np.zeros((3, 160), np.int16))
        with pytest.raises(ValueError, match="CUDA int16"):
            st.push_torch(torch.zeros((2, 160), dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError, match="one value per stream"):
            st.push(np.zeros((2, 160), np.int16), counts=[1])
        with pytest.raises(_lib.DssError, match="stream 1 is to take 3"):
            st.push(np.zeros((2, 320), np.int16), counts=[2, 3])
        with pytest.raises(_lib.DssError, match="stream 0 is to take -1"):
            st.push(np.zeros((2, 320), np.int16), counts=[-1, 2])
        with pytest.raises(_lib.DssError, match="in a reset"):
            st.reset([2])
        with pytest.raises(_lib.DssError, match="in a reset"):
            st.reset([0, -1])
        # no-ops: no frames, or every stream sitting out
        assert st.push(np.zeros((2, 0), np.int16)).shape == (2, 0, 20)
        assert not st.push(np.full((2, 320), JUNK, np.int16), counts=[0, 0], total=True).any()
        assert st.frames_seen.tolist() == [4, 4]
        rest = st.push(np.stack([sig[4 * FRAME:]] * 2), total=True)     # the handle is as good as before, its state untouched
        for s in range(2):
            assert np.array_equal(np.concatenate([half[s], rest[s]]), whole["square"])
    finally:
        st.close()
