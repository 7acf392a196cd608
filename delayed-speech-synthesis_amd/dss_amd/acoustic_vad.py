"""Acoustic (energy based) voice-activity labels for the trials of a recording, on the GPU.

The ``vad_labels`` of the training corpus (``prepare_corpus.get_vad_labels``, prepare_corpus.py:78-116) come from a fresh
``EnergyBasedVad`` per trial (local/common.py:556-649): frames of 50 ms every 10 ms, Hann window, magnitude spectrum, a
40-band mel filter bank (``MelFilterBank``, common.py:475-514), the log energy of every frame, a threshold from the trial's
mean log energy and a vote over neighbouring frames.  ``AcousticVadGPU.labels_trials`` does that for a whole trial list in
two launches (csrc/acoustic_vad.hip) on audio that crosses the bus once.

The audio is taken *as the caller hands it over*: the reference also normalises the loudness of every non-silence trial
through ``pydub`` (``prepare_corpus._normalize_audio``) before it labels it, and that step is not part of this package.  Pass
the raw session wav, or your own normalised trial audio concatenated, plus one ``(first sample, length)`` range per trial.

The window and the mel matrix are computed here, from their definitions, and handed to the library as data.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np

from . import _lib


class AvadParams(C.Structure):
    """dss_avad_params of include/dss_hip.h."""
    _fields_ = [("window", C.c_int), ("shift", C.c_int), ("n_bins", C.c_int), ("n_bands", C.c_int),
                ("frames_context", C.c_int), ("reserved", C.c_int), ("energy_threshold", C.c_double),
                ("energy_mean_scale", C.c_double), ("proportion_threshold", C.c_double)]


def hann(n: int) -> np.ndarray:
    """The symmetric Hann window 0.5 - 0.5 cos(2 pi k / (n - 1)) as numpy evaluates it (``numpy.hanning``; what the
    reference's ``scipy.hanning`` was)."""
    return np.hanning(int(n))


def mel_filterbank(n_bins: int, n_bands: int, fs: float) -> np.ndarray:
    """(n_bins, n_bands) float64 triangular mel filters with unit column sums.

    ``n_bands + 2`` edges equally spaced on the mel scale 2595 log10(1 + f / 700) between 0 and the mel of fs / 2; every edge
    goes back to Hz, is floored, and becomes the bin floor(f / (fs / 2) * n_bins); band i rises linearly over
    [edge_i, edge_i+1) and falls over [edge_i+1, edge_i+2); every band is divided by its own sum (1 where that is 0) and
    non-finite entries become 0."""
    n_bins, n_bands = int(n_bins), int(n_bands)
    nyquist = fs / 2.0
    mel_step = (2595.0 * math.log10(1.0 + nyquist / 700.0)) / (n_bands + 1)
    edges = []
    for k in range(n_bands + 2):
        hz = math.floor(700.0 * (math.pow(10.0, (k * mel_step) / 2595.0) - 1.0))
        edges.append(int(math.floor((hz / nyquist) * n_bins)))
    bank = np.zeros((n_bands, n_bins), dtype=np.float64)
    for i in range(n_bands):
        lo, mid, hi = edges[i:i + 3]
        bank[i, lo:mid] = (np.arange(lo, mid) - lo) / float(mid - lo) if mid > lo else 0.0
        bank[i, mid:hi] = (hi - np.arange(mid, hi)) / float(hi - mid) if hi > mid else 0.0
    sums = bank.sum(axis=1)
    sums[sums == 0] = 1.0
    out = bank / sums[:, None]
    out[~np.isfinite(out)] = 0.0
    return np.ascontiguousarray(out.T)


def trial_frames(n: int, window: int = 800, shift: int = 160) -> int:
    """floor((n - window) / shift) + 1; DssError for a trial shorter than one window (needs no GPU)."""
    return _lib.check(_lib.load().dss_avad_trial_frames_for(int(n), int(window), int(shift)))


def _trial_arrays(ranges, lead):
    t = np.asarray(list(ranges), dtype=np.int64).reshape(-1, 2)
    if np.any(np.abs(t[:, 1]) > 2**31 - 1):
        raise _lib.DssError("trial length does not fit 32 bits")
    ld = np.broadcast_to(np.asarray(lead, dtype=np.int64), (len(t),))
    if np.any(np.abs(ld) > 2**31 - 1):
        raise _lib.DssError("lead does not fit 32 bits")
    return (np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1].astype(np.int32)),
            np.ascontiguousarray(ld.astype(np.int32)))


def check_trials(n_audio: int, ranges, lead=0, window: int = 800, shift: int = 160) -> int:
    """The argument checks of ``labels_trials`` on their own: total frames of ``[(first, length)]`` in audio of ``n_audio``
    samples; DssError with the reason otherwise (needs no GPU)."""
    first, length, ld = _trial_arrays(ranges, lead)
    return _lib.check(_lib.load().dss_avad_check_trials(int(n_audio), len(first), first.ctypes.data, length.ctypes.data,
                                                        ld.ctypes.data, int(window), int(shift)))


def vote_host(log_energy, energy_threshold=4.0, energy_mean_scale=1.0, frames_context: int = 5,
              proportion_threshold: float = 0.6):
    """Threshold and vote of ONE trial from its log energies, on the host (dss_avad_vote_host; needs no GPU):
    ``(labels bool (W,), threshold)``."""
    le = np.ascontiguousarray(log_energy, dtype=np.float64).reshape(-1)
    p = AvadParams(0, 0, 0, 0, int(frames_context), 0, float(energy_threshold), float(energy_mean_scale),
                   float(proportion_threshold))
    labels = np.zeros(len(le), dtype=np.uint8)
    thr = C.c_double(0.0)
    _lib.check(_lib.load().dss_avad_vote_host(le.ctypes.data, len(le), C.addressof(p), labels.ctypes.data, C.addressof(thr)))
    return labels.astype(bool), thr.value


class AcousticVadGPU:
    """EnergyBasedVad(energy_threshold, energy_mean_scale, frames_context, proportion_threshold).from_wav for trial lists."""

    def __init__(self, fs: int = 16000, window_length: float = 0.05, frame_shift: float = 0.01, n_bands: int = 40,
                 energy_threshold: float = 4, energy_mean_scale: float = 1, frames_context: int = 5,
                 proportion_threshold: float = 0.6):
        self.fs = int(fs)
        self.window = int(self.fs * window_length)
        self.shift = int(self.fs * frame_shift)
        self.n_bins = self.window // 2 + 1
        self.params = AvadParams(self.window, self.shift, self.n_bins, int(n_bands), int(frames_context), 0,
                                 float(energy_threshold), float(energy_mean_scale), float(proportion_threshold))
        L = _lib.load()
        _lib.check(L.dss_avad_check_params(C.addressof(self.params)))
        L = _lib.require_gpu()
        self._L = L
        self.window_fn = np.ascontiguousarray(hann(self.window), dtype=np.float64)
        self.mel = np.ascontiguousarray(mel_filterbank(self.n_bins, int(n_bands), self.fs), dtype=np.float64)
        self._h = L.dss_avad_create(C.addressof(self.params), self.window_fn.ctypes.data, self.mel.ctypes.data)
        if not self._h:
            raise _lib.DssError(L.dss_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.dss_avad_destroy(self._h)
            self._h = None

    __del__ = close

    def trial_frames(self, n: int) -> int:
        return trial_frames(n, self.window, self.shift)

    def _args(self, n_audio, ranges, lead, silence):
        first, length, ld = _trial_arrays(ranges, lead)
        total = _lib.check(self._L.dss_avad_check_trials(int(n_audio), len(first), first.ctypes.data, length.ctypes.data,
                                                         ld.ctypes.data, self.window, self.shift))
        sil = None
        if silence is not None:
            sil = np.ascontiguousarray(np.asarray(silence).astype(bool).astype(np.uint8).reshape(-1))
            if len(sil) != len(first):
                raise ValueError("silence must hold one flag per trial")
        return first, length, ld, sil, total

    def labels_trials(self, audio: np.ndarray, ranges, lead=0, silence: Optional[Sequence[bool]] = None,
                      return_energy: bool = False):
        """``audio`` int16 (n,) host, as the caller hands it over (no loudness normalisation is applied); ``ranges``
        [(first sample, length)]: trial i is ``lead`` zeros followed by ``audio[first : first + length - lead]`` (the
        reference's 16 ms shift is ``lead=256``); ``silence``: trials that get all-zero labels.  Returns bool (sum W_i,)
        labels, trial after trial in list order; with ``return_energy`` also the float64 log energies (sum W_i,) and the
        thresholds (n_trials,)."""
        a = np.asarray(audio)
        if a.dtype != np.int16 or a.ndim != 1:
            raise ValueError("audio must be a one-dimensional int16 array")
        a = np.ascontiguousarray(a)
        first, length, ld, sil, total = self._args(len(a), ranges, lead, silence)
        labels = np.zeros(total, dtype=np.uint8)
        le = np.zeros(total, dtype=np.float64) if return_energy else None
        thr = np.zeros(len(first), dtype=np.float64) if return_energy else None
        if total:
            got = _lib.check(self._L.dss_avad_labels_trials(
                self._h, a.ctypes.data, len(a), len(first), first.ctypes.data, length.ctypes.data, ld.ctypes.data,
                sil.ctypes.data if sil is not None else None, labels.ctypes.data,
                le.ctypes.data if return_energy else None, thr.ctypes.data if return_energy else None))
            assert got == total
        return (labels.astype(bool), le, thr) if return_energy else labels.astype(bool)

    def labels_trials_torch(self, audio, ranges, lead=0, silence: Optional[Sequence[bool]] = None,
                            return_energy: bool = False, stream=None):
        """Device-resident form: CUDA int16 (n,) tensor -> CUDA uint8 (sum W_i,) labels (and float64 log energies and
        thresholds); queued on the current (or the given) stream, no synchronisation.  The same audio contract as
        ``labels_trials``."""
        import torch
        assert audio.is_cuda and audio.dtype == torch.int16 and audio.is_contiguous() and audio.dim() == 1
        first, length, ld, sil, total = self._args(audio.shape[0], ranges, lead, silence)
        dev = audio.device
        labels = torch.empty(total, dtype=torch.uint8, device=dev)
        le = torch.empty(total, dtype=torch.float64, device=dev) if return_energy else None
        thr = torch.empty(len(first), dtype=torch.float64, device=dev) if return_energy else None
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        if total:
            got = _lib.check(self._L.dss_avad_labels_trials_dev(
                self._h, audio.data_ptr(), audio.shape[0], len(first), first.ctypes.data, length.ctypes.data, ld.ctypes.data,
                sil.ctypes.data if sil is not None else None, labels.data_ptr(),
                le.data_ptr() if return_energy else None, thr.data_ptr() if return_energy else None, s))
            assert got == total
        return (labels, le, thr) if return_energy else labels
