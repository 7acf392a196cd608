"""Lifetimes of the device memory behind the C ABI's handles (DssDevBlocks, csrc/dss_host.h): the paths on which a handle frees
and allocates again while it lives, which no other test walks on one handle.

Every comparison is bit-exact (np.array_equal / torch.equal) against the same call on a freshly created handle: a buffer that
was freed too early, re-allocated too small or left dangling shows as a difference (or as a fault), and nothing else can differ,
because both handles run the same kernels on the same input.

Grow, then reuse: a small call, a larger one, the small one again.  The larger call is sized so that every buffer whose size
follows the data (staging, outputs, workspaces) is allocated again; the tables of 9 trial descriptors of the analysis handles
fit in the headroom of the first allocation (64 spare entries), which is the other path: reuse without allocating."""
import ctypes as C

import numpy as np
import pytest
import torch

from dss_amd.synthetic import synthetic_ecog, synthetic_speech_audio

pytestmark = pytest.mark.gpu


def _grow_then_reuse(make, call, small, large, equal=np.array_equal):
    """make() -> handle; call(handle, case) -> result.  small, large, small on one handle against a fresh handle each."""
    used = make()
    got = [call(used, case) for case in (small, large, small)]
    for case, g in zip((small, large, small), got):
        assert equal(g, call(make(), case))


def _trials(n, first_len, step, stride):
    return [(i * stride, first_len + (i % 3) * step) for i in range(n)]


def test_hga_trial_lists_grow_then_reuse():
    from dss_amd.hga import HgaExtractorGPU
    rec = synthetic_ecog(31, 4000, 4)
    _grow_then_reuse(lambda: HgaExtractorGPU(1, 4), lambda h, tr: h.extract_trials(rec, tr),
                     _trials(2, 60, 15, 70), _trials(9, 300, 40, 400))


def test_hga_trial_lists_with_patches_and_zscore_grow_then_reuse():
    """The patched form adds the table of one-frame trials; set_patches / set_zscore free and upload again when called twice."""
    from dss_amd.hga import HgaExtractorGPU
    rec = synthetic_ecog(32, 4000, 5)

    def make():
        h = HgaExtractorGPU(1, 5)
        for scale in (2.0, 1.0):                           # the second call replaces the first one's device copies
            h.set_patches([(1, [0, 2]), (4, [3, 2, 0])] if scale == 1.0 else [(0, [1])])
            h.set_zscore(np.arange(5) * scale, 1.0 + np.arange(5) * scale)
        return h

    def call(h, tr):
        return h.extract_trials_torch(torch.from_numpy(rec).cuda(), tr).cpu().numpy()

    small = [(0, 40), (100, 60)]                           # the first emits one frame: the table of single-frame trials
    _grow_then_reuse(make, call, small, _trials(9, 300, 40, 400) + [(3900, 30)])


def test_acoustic_vad_grow_then_reuse():
    from dss_amd.acoustic_vad import AcousticVadGPU
    wav = synthetic_speech_audio(33, 60000)

    def call(v, tr):
        labels, le, thr = v.labels_trials(wav, tr, lead=16, return_energy=True)
        return np.concatenate([labels.astype(np.float64), le, thr])

    _grow_then_reuse(AcousticVadGPU, call, _trials(2, 800, 160, 900), _trials(9, 4000, 480, 6000))


def test_spectrogram_trials_grow_then_reuse():
    from dss_amd.spectral import SpectrogramGPU
    x = synthetic_ecog(34, 6000, 3)
    _grow_then_reuse(lambda: SpectrogramGPU(1000, 16, 8), lambda s, tr: s.trials(x, tr),
                     _trials(2, 16, 8, 20), _trials(9, 400, 50, 600))


def test_contamination_grow_then_reuse():
    """No trial list here: the recording grows (the audio spectrogram, the frame mask and the staging follow its length)."""
    from dss_amd.contamination import ContaminationGPU
    brain = synthetic_ecog(35, 4000, 3)
    audio = synthetic_ecog(36, 4000, 1)[:, 0]

    def call(h, n_rows):
        m = h.moments(brain[:n_rows], audio[:n_rows])
        return np.concatenate([np.asarray(f, dtype=np.float64).reshape(-1) for f in m])

    _grow_then_reuse(lambda: ContaminationGPU(1000, max_lag=0.1), call, 300, 4000,
                     equal=lambda a, b: np.array_equal(a, b, equal_nan=True))


def _vad_sd(seed, C_=5, H=6):
    rng = np.random.default_rng(seed)
    shapes = [(4 * H, C_), (4 * H, H), (4 * H,), (4 * H,), (4 * H, H), (4 * H, H), (4 * H,), (4 * H,), (2, H), (2,)]
    from dss_amd.vad import _KEYS
    return {k: rng.uniform(-0.5, 0.5, s).astype(np.float32) for k, s in zip(_KEYS, shapes)}


def _dec_sd(seed, C_=5, H=6, O=3):
    rng = np.random.default_rng(seed)
    shapes = []
    for layer in (0, 1):
        for _ in range(2):
            shapes += [(4 * H, 2 * H if layer else C_), (4 * H, H), (4 * H,), (4 * H,)]
    shapes += [(O, 2 * H), (O,)]
    from dss_amd.decoder import _KEYS
    return {k: rng.uniform(-0.5, 0.5, s).astype(np.float32) for k, s in zip(_KEYS, shapes)}


def _frames(seed, n, C_=5):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, C_)).astype(np.float32)).cuda()


def test_vad_trial_lists_grow_then_reuse():
    from dss_amd.vad import VadLstmGPU
    x = _frames(41, 200)

    def call(v, tr):
        labels, logits = v.forward_trials_torch(x, tr, want_logits=True)
        return torch.cat([labels.to(torch.float32).reshape(-1), logits.reshape(-1)])

    _grow_then_reuse(lambda: VadLstmGPU(1, state_dict=_vad_sd(1)), call, _trials(2, 3, 2, 5), _trials(9, 8, 3, 20), equal=torch.equal)


def test_decoder_trial_lists_grow_then_reuse():
    """max_streams 2: the 9 trials also run as five chunks over the handle's layer buffers."""
    from dss_amd.decoder import BiLstmDecoderGPU
    x = _frames(42, 200)
    _grow_then_reuse(lambda: BiLstmDecoderGPU(2, 12, state_dict=_dec_sd(2)), lambda d, tr: d.forward_trials_torch(x, tr),
                     _trials(2, 3, 2, 5), _trials(9, 8, 2, 20), equal=torch.equal)


def test_vad_weight_reload():
    """Weights A, run, weights B, run: the arrays of A are freed behind the switch, and the second result is B's."""
    from dss_amd import _lib
    from dss_amd.vad import _KEYS, VadLstmGPU
    x = _frames(43, 8)[None]
    a, b = _vad_sd(11), _vad_sd(12)
    v = VadLstmGPU(1, state_dict=a)
    _, with_a = v.step_torch(x, want_logits=True)
    _lib.check(v._L.dss_vad_load_weights(v._h, *[b[k].ctypes.data for k in _KEYS]))
    v.reset()
    _, got = v.step_torch(x, want_logits=True)
    _, want = VadLstmGPU(1, state_dict=b).step_torch(x, want_logits=True)
    assert torch.equal(got, want) and not torch.equal(got, with_a)


def test_decoder_weight_reload():
    from dss_amd import _lib
    from dss_amd.decoder import _KEYS, BiLstmDecoderGPU
    x = _frames(44, 8)[None]
    a, b = _dec_sd(21), _dec_sd(22)
    d = BiLstmDecoderGPU(1, 8, state_dict=a)
    with_a = d(x)
    _lib.check(d._L.dss_dec_load_weights(d._h, (C.c_void_p * 18)(*[b[k].ctypes.data for k in _KEYS])))
    got = d(x)
    assert torch.equal(got, BiLstmDecoderGPU(1, 8, state_dict=b)(x)) and not torch.equal(got, with_a)


def test_batch_trace_resize():
    """Teacher forcing at 2 frames, then at 4: the forced excitation and the logit trace are freed and allocated again at the new
    shape, beside the trace buffers that enable_trace allocated late; then back to free running on the same batch."""
    from dss_amd import lpcnet
    from dss_amd.lpcnet_weights import synthetic_blob, synthetic_features
    lpcnet.load_model(synthetic_blob(0))
    feats = np.stack([synthetic_features(60 + u, 4) for u in range(2)])
    exc = np.clip(np.rint(128 + np.random.default_rng(45).normal(0, 30, (2, 4 * 160))), 0, 255).astype(np.uint8)

    def forced(b, F):
        b.force_excitation(exc[:, :F * 160], F)
        b.reset()
        pcm = b.synthesize(feats[:, :F])
        return [pcm] + [b.tap(u, which, F) for u in range(2) for which in (3, 4, 5)]

    used = lpcnet.LPCNetBatch(2, 4)
    used.enable_trace(1)
    at2 = forced(used, 2)
    at4 = forced(used, 4)
    used.force_excitation(None, 0)
    used.reset()
    free = used.synthesize(feats)
    for F, got in ((2, at2), (4, at4)):
        fresh = lpcnet.LPCNetBatch(2, 4)
        fresh.enable_trace(1)
        for g, w in zip(got, forced(fresh, F)):
            assert np.array_equal(g, w), F
    assert np.array_equal(free, lpcnet.LPCNetBatch(2, 4).synthesize(feats))


def test_failed_create_leaves_the_library_usable():
    """A refused create returns NULL with a message, and the next valid create of the same kind works.  The spectrogram's is
    refused after the handle exists (its destroy runs on a handle that owns nothing yet)."""
    from dss_amd import _lib
    from dss_amd.decoder import BiLstmDecoderGPU
    from dss_amd.gate import SpeechGateGPU
    from dss_amd.spectral import SpectrogramGPU
    from dss_amd.vad import VadLstmGPU
    L = _lib.require_gpu()
    assert not L.dss_vad_create(1, 5, 100000) and b"out of range" in L.dss_last_error()
    assert VadLstmGPU(1, state_dict=_vad_sd(1)).step_torch(_frames(46, 8)[None]).shape == (1, 8)
    assert not L.dss_dec_create(1, 8, 5, 100000, 3) and b"out of range" in L.dss_last_error()
    assert BiLstmDecoderGPU(1, 8, state_dict=_dec_sd(2))(_frames(47, 8)[None]).shape == (1, 8, 3)
    with pytest.raises(_lib.DssError, match="<= 64"):
        SpeechGateGPU(1, 4, 32, 2, 40)
    assert SpeechGateGPU(1, 4, 32, 2, 1).E > 0
    with pytest.raises(_lib.DssError, match="the window is all zero"):
        SpectrogramGPU(1000, 16, 8, window=np.zeros(16))
    assert SpectrogramGPU(1000, 16, 8).trials(synthetic_ecog(48, 64, 3), [(0, 32)]).shape == (3, 3, 9)
