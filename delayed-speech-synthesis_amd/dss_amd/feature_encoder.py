"""The LPC feature encoder on the GPU (Part 16 of include/dss_hip.h): what ``prepare_corpus.get_lpc_coefficients`` runs
xiph's ``LPCFeatureEncoder`` for (prepare_corpus.py:55-76, LPCNet.pyx:65-87), over a whole trial list in one call.

The method is this project's statement of the published encoder (the binding definition is
tests/feature_encoder_reference.py); parity with xiph's code is not pinned.  One fresh encoder per trial, no LPCNet model
needed.  Per 160-sample frame: 18 Bark cepstral coefficients, the pitch feature and correlation as the decoder reads them
(together the 20 values ``LPCNet.synthesize`` takes) and the 16 LPC taps the decoder derives from that cepstrum.

``LpcFeatureStreamsGPU`` (Part 18) is the same encoder with its state carried from push to push, for audio that arrives in
pieces: any chunking of a stream gives the bits of the whole signal as one trial.  Whole trials stay with ``features_trials``.
"""
from __future__ import annotations

import numpy as np

from . import _lib

FRAME_SIZE = 160
NB_FEATURES = 20
NB_TOTAL_FEATURES = 36
N_LAGS = 256


def frame_offsets(offsets) -> np.ndarray:
    """int64 (n_trials + 1,): the first output frame of every trial and the total (dss_fenc_frame_offsets; needs no GPU)."""
    offs = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if len(offs) < 1:
        raise ValueError("offsets must hold n_trials + 1 values")
    out = np.zeros(len(offs), dtype=np.int64)
    _lib.check(_lib.load().dss_fenc_frame_offsets(offs.ctypes.data, len(offs) - 1, out.ctypes.data))
    return out


class LpcFeatureEncoderGPU:
    NB_FEATURES: int = NB_FEATURES
    NB_TOTAL_FEATURES: int = NB_TOTAL_FEATURES
    LPCNET_FRAME_SIZE: int = FRAME_SIZE

    def __init__(self):
        L = _lib.require_gpu()
        self._L = L
        self._h = L.dss_fenc_create()
        if not self._h:
            raise _lib.DssError(L.dss_last_error().decode())
        self._subframes = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.dss_fenc_destroy(self._h)
            self._h = None

    __del__ = close

    @staticmethod
    def _offsets(offsets) -> np.ndarray:
        offs = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(offs) < 1:
            raise ValueError("offsets must hold n_trials + 1 values")
        return offs

    def features_trials(self, audio: np.ndarray, offsets, total: bool = False):
        """int16 concatenation + offsets (what ``session_trial_audio`` returns) -> ``(float32 (F, 20 | 36), frame_offsets)``:
        trial i's frames are rows ``frame_offsets[i] : frame_offsets[i + 1]``.  ``total``: all 36 values (with the LPC taps)."""
        audio = np.asarray(audio)
        if audio.ndim != 1 or audio.dtype != np.int16:
            raise ValueError("audio must be a one-dimensional int16 array")
        audio = np.ascontiguousarray(audio)
        offs = self._offsets(offsets)
        fo = frame_offsets(offs)
        out = np.zeros((int(fo[-1]), NB_TOTAL_FEATURES), dtype=np.float32)
        got = _lib.check(self._L.dss_fenc_features_trials(self._h, audio.ctypes.data, len(audio), offs.ctypes.data, len(offs) - 1,
                                                          out.ctypes.data))
        assert got == fo[-1]
        self._subframes = 2 * int(got)
        return (out if total else np.ascontiguousarray(out[:, :NB_FEATURES])), fo

    def features_trials_torch(self, audio, offsets, total: bool = False, stream=None):
        """Device-resident form: CUDA int16 (n,) -> ``(CUDA float32 (F, 20 | 36), frame_offsets)``; queued on the current (or the
        given) stream, no synchronisation.  ``offsets`` is a host sequence."""
        import torch
        if not (isinstance(audio, torch.Tensor) and audio.is_cuda and audio.dtype == torch.int16 and audio.dim() == 1):
            raise ValueError("audio must be a one-dimensional CUDA int16 tensor")
        audio = audio.contiguous()
        offs = self._offsets(offsets)
        fo = frame_offsets(offs)
        dev = audio.device
        out = torch.zeros((int(fo[-1]), NB_TOTAL_FEATURES), dtype=torch.float32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        got = _lib.check(self._L.dss_fenc_features_trials_dev(self._h, audio.data_ptr(), audio.shape[0], offs.ctypes.data, len(offs) - 1,
                                                              out.data_ptr(), s))
        assert got == fo[-1]
        self._subframes = 2 * int(got)
        return (out if total else out[:, :NB_FEATURES].contiguous()), fo

    def compute_LPC_features(self, audio_samples: np.ndarray) -> np.ndarray:
        """``LPCFeatureEncoder.compute_LPC_features`` (LPCNet.pyx:65-87) for one trial: int16[n] -> float32[n // 160, 20], with
        the Cython signature's buffer checks."""
        if not isinstance(audio_samples, np.ndarray):
            raise TypeError("Argument 'audio_samples' has incorrect type (expected numpy.ndarray, got %s)"
                            % type(audio_samples).__name__)
        if audio_samples.ndim != 1:
            raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % audio_samples.ndim)
        if audio_samples.dtype != np.int16:
            raise ValueError("Buffer dtype mismatch, expected 'int16_t' but got '%s'" % audio_samples.dtype.name)
        return self.features_trials(audio_samples, [0, len(audio_samples)])[0]

    def enable_timing(self, on: bool = True) -> None:
        """Development timing: events around the three launches of every later call (no synchronisation)."""
        _lib.check(self._L.dss_fenc_enable_timing(self._h, int(bool(on))))

    def kernel_ms(self):
        """Device time in ms of the last timed call's three launches (spectrum, scores, track); waits for that call."""
        ms = [self._L.dss_fenc_kernel_ms(self._h, k) for k in range(3)]
        if min(ms) < 0:
            raise _lib.DssError(self._L.dss_last_error().decode())
        return ms

    def scores(self) -> np.ndarray:
        """The score scratch of the last call (the tests' tap): float64 (2 F, 256); columns 0..254 the damped normalised
        cross-correlations at lag 256 - column, column 255 the sub-frame's normalised weight."""
        out = np.zeros((self._subframes, N_LAGS), dtype=np.float64)
        _lib.check(self._L.dss_fenc_tap_scores(self._h, out.ctypes.data, out.size))
        return out


def streams_check(n_streams: int, frames_max: int, counts=None) -> int:
    """The argument checks of a push (dss_fenc_streams_check; needs no GPU): the number of frames it would encode."""
    c = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if c is not None and len(c) != n_streams:
        raise ValueError("counts must hold one value per stream")
    return _lib.check(_lib.load().dss_fenc_streams_check(int(n_streams), int(frames_max), None if c is None else c.ctypes.data))


class LpcFeatureStreamsGPU:
    """The same encoder on ``n_streams`` streams whose state is carried from push to push (Part 18 of include/dss_hip.h): any
    chunking of a stream gives, bit for bit, what ``LpcFeatureEncoderGPU.features_trials`` gives on the whole signal as one
    trial.  One launch per push."""
    NB_FEATURES: int = NB_FEATURES
    NB_TOTAL_FEATURES: int = NB_TOTAL_FEATURES
    LPCNET_FRAME_SIZE: int = FRAME_SIZE

    def __init__(self, n_streams: int):
        L = _lib.load()
        self._L = L
        self._h = None
        self.n_streams = int(n_streams)
        _lib.check(L.dss_fenc_streams_check(self.n_streams, 0, None))
        _lib.require_gpu()
        self._h = L.dss_fenc_streams_create(self.n_streams)
        if not self._h:
            raise _lib.DssError(L.dss_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.dss_fenc_streams_destroy(self._h)
            self._h = None

    __del__ = close

    def _counts(self, counts):
        if counts is None:
            return None
        c = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        if len(c) != self.n_streams:
            raise ValueError("counts must hold one value per stream")
        return c

    def _shape(self, shape) -> int:
        if len(shape) != 2 or shape[0] != self.n_streams or shape[1] % FRAME_SIZE:
            raise ValueError("audio must be int16 (n_streams, 160 k)")
        return shape[1] // FRAME_SIZE

    def push(self, audio: np.ndarray, counts=None, total: bool = False) -> np.ndarray:
        """int16 (S, 160 K), ``counts`` (S,) frames per stream or None for K each -> float32 (S, K, 20 | 36); the rows past a
        stream's count are zeros, and a count of 0 leaves that stream's state untouched."""
        audio = np.asarray(audio)
        if audio.ndim != 2 or audio.dtype != np.int16:
            raise ValueError("audio must be a two-dimensional int16 array")
        K = self._shape(audio.shape)
        audio = np.ascontiguousarray(audio)
        c = self._counts(counts)
        out = np.zeros((self.n_streams, K, NB_TOTAL_FEATURES), dtype=np.float32)
        _lib.check(self._L.dss_fenc_streams_push(self._h, audio.ctypes.data, K, None if c is None else c.ctypes.data, out.ctypes.data))
        return out if total else np.ascontiguousarray(out[:, :, :NB_FEATURES])

    def push_torch(self, audio, counts=None, total: bool = False, stream=None):
        """Device-resident form: CUDA int16 (S, 160 K) -> CUDA float32 (S, K, 20 | 36), queued on the current (or the given)
        stream, no synchronisation.  ``counts`` is a host sequence."""
        import torch
        if not (isinstance(audio, torch.Tensor) and audio.is_cuda and audio.dtype == torch.int16 and audio.dim() == 2):
            raise ValueError("audio must be a two-dimensional CUDA int16 tensor")
        K = self._shape(tuple(audio.shape))
        audio = audio.contiguous()
        c = self._counts(counts)
        dev = audio.device
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        # the launch writes every row, zeros past the counts included, in the stream's order; a no-op writes nothing
        out = torch.empty((self.n_streams, K, NB_TOTAL_FEATURES), dtype=torch.float32, device=dev)
        got = _lib.check(self._L.dss_fenc_streams_push_dev(self._h, audio.data_ptr(), K, None if c is None else c.ctypes.data,
                                                           out.data_ptr(), s))
        if got == 0:
            out.zero_()
        return out if total else out[:, :, :NB_FEATURES].contiguous()

    def reset(self, streams=None, stream=None) -> None:
        """The listed streams (None: all) back to the fresh state, in order on the null (or the given raw) stream."""
        if streams is None:
            _lib.check(self._L.dss_fenc_streams_reset(self._h, None, 0, stream))
            return
        idx = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
        _lib.check(self._L.dss_fenc_streams_reset(self._h, idx.ctypes.data, len(idx), stream))

    @property
    def frames_seen(self) -> np.ndarray:
        """int64 (S,): frames every stream has encoded since its reset."""
        out = np.zeros(self.n_streams, dtype=np.int64)
        _lib.check(self._L.dss_fenc_streams_frames_seen(self._h, out.ctypes.data))
        return out
