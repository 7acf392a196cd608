"""Acoustic (energy based) voice-activity labels for the trials of a recording, on the GPU.

The ``vad_labels`` of the training corpus (``prepare_corpus.get_vad_labels``, prepare_corpus.py:78-116) come from a fresh
``EnergyBasedVad`` per trial (local/common.py:556-649): frames of 50 ms every 10 ms, Hann window, magnitude spectrum, a
40-band mel filter bank (``MelFilterBank``, common.py:475-514), the log energy of every frame, a threshold from the trial's
mean log energy and a vote over neighbouring frames.  ``AcousticVadGPU.labels_trials`` does that for a whole trial list in
two launches (csrc/acoustic_vad.hip) on audio that crosses the bus once.

By default the audio is taken *as the caller hands it over*.  The reference also normalises the loudness of every non-silence
trial through ``pydub`` (``prepare_corpus._normalize_audio``) before it labels it; that step is opt-in here: ``set_gain()`` and
``normalize=True`` give the labels of the audio as the reference prepares it (a peak launch in front, the two gains applied
as the energy kernel stages its samples), and ``prepared_audio_trials`` returns that audio itself, which is what the
reference's feature encoder is given.  The arithmetic is pinned by tests/golden/trial_audio.npz (Python's own ``audioop``);
the gain table is data from ``dss_amd.trial_audio``.  Pass the raw session wav plus one ``(first sample, length)`` range per
trial.

The window and the mel matrix are computed here, from their definitions, and handed to the library as data.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import numpy as np

from . import _lib, trial_audio


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

    def set_gain(self, table=None, post: Optional[float] = None):
        """The loudness step's data: ``table`` float64 (32769,) factor by peak (default ``trial_audio.pydub_gain_table()``:
        pydub's ``effects.normalize`` at 0.1 dB headroom) and the ``post`` factor (default ``trial_audio.post_gain()``: -3 dB).
        Uploaded once; DssError for a negative or non-finite entry."""
        t = np.ascontiguousarray(trial_audio.pydub_gain_table() if table is None else table, dtype=np.float64).reshape(-1)
        if len(t) != trial_audio.N_PEAKS:
            raise ValueError("the gain table holds one factor per peak 0 .. 32768")
        _lib.check(self._L.dss_avad_set_gain(self._h, t.ctypes.data, float(trial_audio.post_gain() if post is None else post)))
        self._gain_set = True

    def _normalize_flags(self, normalize, sil, n_trials):
        """None -> None; True -> every trial that is not silent; a sequence -> one flag per trial."""
        if normalize is None:
            return None
        if isinstance(normalize, (bool, np.bool_)):
            flags = np.full(n_trials, bool(normalize))
            if sil is not None:
                flags &= ~sil.astype(bool)
        else:
            flags = np.asarray(normalize).astype(bool).reshape(-1)
            if len(flags) != n_trials:
                raise ValueError("normalize must hold one flag per trial")
        if flags.any() and not getattr(self, "_gain_set", False):
            self.set_gain()
        return np.ascontiguousarray(flags.astype(np.uint8))

    def labels_trials(self, audio: np.ndarray, ranges, lead=0, silence: Optional[Sequence[bool]] = None,
                      return_energy: bool = False, normalize=None):
        """``audio`` int16 (n,) host, as the caller hands it over (no loudness normalisation unless ``normalize``); ``ranges``
        [(first sample, length)]: trial i is ``lead`` zeros followed by ``audio[first : first + length - lead]`` (the
        reference's 16 ms shift is ``lead=256``); ``silence``: trials that get all-zero labels.  Returns bool (sum W_i,)
        labels, trial after trial in list order; with ``return_energy`` also the float64 log energies (sum W_i,) and the
        thresholds (n_trials,).  ``normalize``: None is the plain call; True labels every trial that is not silent on its
        audio as the reference prepares it (module docstring; ``set_gain`` with the pydub defaults unless called before); a
        sequence flags the trials one by one."""
        a = np.asarray(audio)
        if a.dtype != np.int16 or a.ndim != 1:
            raise ValueError("audio must be a one-dimensional int16 array")
        a = np.ascontiguousarray(a)
        first, length, ld, sil, total = self._args(len(a), ranges, lead, silence)
        labels = np.zeros(total, dtype=np.uint8)
        le = np.zeros(total, dtype=np.float64) if return_energy else None
        thr = np.zeros(len(first), dtype=np.float64) if return_energy else None
        norm = self._normalize_flags(normalize, sil, len(first))
        if total and norm is not None:
            got = _lib.check(self._L.dss_avad_prepare_trials(
                self._h, a.ctypes.data, len(a), len(first), first.ctypes.data, length.ctypes.data, ld.ctypes.data,
                sil.ctypes.data if sil is not None else None, norm.ctypes.data, labels.ctypes.data,
                le.ctypes.data if return_energy else None, thr.ctypes.data if return_energy else None, None, None))
            assert got == total
        elif total:
            got = _lib.check(self._L.dss_avad_labels_trials(
                self._h, a.ctypes.data, len(a), len(first), first.ctypes.data, length.ctypes.data, ld.ctypes.data,
                sil.ctypes.data if sil is not None else None, labels.ctypes.data,
                le.ctypes.data if return_energy else None, thr.ctypes.data if return_energy else None))
            assert got == total
        return (labels.astype(bool), le, thr) if return_energy else labels.astype(bool)

    def labels_trials_torch(self, audio, ranges, lead=0, silence: Optional[Sequence[bool]] = None,
                            return_energy: bool = False, stream=None, normalize=None):
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
        norm = self._normalize_flags(normalize, sil, len(first))
        if total and norm is not None:
            got = _lib.check(self._L.dss_avad_prepare_trials_dev(
                self._h, audio.data_ptr(), audio.shape[0], len(first), first.ctypes.data, length.ctypes.data, ld.ctypes.data,
                sil.ctypes.data if sil is not None else None, norm.ctypes.data, labels.data_ptr(),
                le.data_ptr() if return_energy else None, thr.data_ptr() if return_energy else None, None, None, s))
            assert got == total
        elif total:
            got = _lib.check(self._L.dss_avad_labels_trials_dev(
                self._h, audio.data_ptr(), audio.shape[0], len(first), first.ctypes.data, length.ctypes.data, ld.ctypes.data,
                sil.ctypes.data if sil is not None else None, labels.data_ptr(),
                le.data_ptr() if return_energy else None, thr.data_ptr() if return_energy else None, s))
            assert got == total
        return (labels, le, thr) if return_energy else labels

    def _audio_args(self, ranges, lead, silence, normalize):
        first, length, ld = _trial_arrays(ranges, lead)
        sil = None
        if silence is not None:
            sil = np.ascontiguousarray(np.asarray(silence).astype(bool).astype(np.uint8).reshape(-1))
            if len(sil) != len(first):
                raise ValueError("silence must hold one flag per trial")
        norm = self._normalize_flags(normalize, sil, len(first))
        if np.any(length < 0):
            raise _lib.DssError("negative trial length")
        offsets = np.concatenate([[0], np.cumsum(length.astype(np.int64))])
        return first, length, ld, norm, offsets

    def prepared_audio_trials(self, audio: np.ndarray, ranges, lead=0, normalize=None, return_peaks: bool = False,
                              silence: Optional[Sequence[bool]] = None):
        """The trials' audio as the reference prepares it before anything reads it (prepare_corpus.py:63-69): int16
        (sum length_i,), trial i at ``sum(length[:i])``: ``lead`` zeros, then the first ``length - lead`` samples of the cut
        ``audio[first : first + length]``, of a trial flagged by ``normalize`` scaled by the factor of the cut's peak and by the
        post gain (two roundings, as pydub's two ``audioop.mul``).  ``normalize`` as in ``labels_trials``; ``True`` leaves the
        trials flagged in ``silence`` as they are.  A trial may be shorter than one window.  With ``return_peaks`` also the
        int32 peak of every trial's cut."""
        a = np.asarray(audio)
        if a.dtype != np.int16 or a.ndim != 1:
            raise ValueError("audio must be a one-dimensional int16 array")
        a = np.ascontiguousarray(a)
        first, length, ld, norm, offsets = self._audio_args(ranges, lead, silence, normalize)
        out = np.zeros(int(offsets[-1]), dtype=np.int16)
        peaks = np.zeros(len(first), dtype=np.int32)
        if len(first):
            _lib.check(self._L.dss_avad_prepare_trials(
                self._h, a.ctypes.data, len(a), len(first), first.ctypes.data, length.ctypes.data, ld.ctypes.data, None,
                norm.ctypes.data if norm is not None else None, None, None, None, out.ctypes.data,
                peaks.ctypes.data if return_peaks else None))
        return (out, peaks) if return_peaks else out

    def prepared_audio_trials_torch(self, audio, ranges, lead=0, normalize=None, return_peaks: bool = False,
                                    silence: Optional[Sequence[bool]] = None, stream=None):
        """Device-resident form of ``prepared_audio_trials``: CUDA int16 (n,) -> CUDA int16 (sum length_i,) (and CUDA int32
        peaks); queued on the current (or the given) stream, no synchronisation."""
        import torch
        assert audio.is_cuda and audio.dtype == torch.int16 and audio.is_contiguous() and audio.dim() == 1
        first, length, ld, norm, offsets = self._audio_args(ranges, lead, silence, normalize)
        dev = audio.device
        out = torch.empty(int(offsets[-1]), dtype=torch.int16, device=dev)
        peaks = torch.empty(len(first), dtype=torch.int32, device=dev) if return_peaks else None
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        if len(first):
            _lib.check(self._L.dss_avad_prepare_trials_dev(
                self._h, audio.data_ptr(), audio.shape[0], len(first), first.ctypes.data, length.ctypes.data, ld.ctypes.data, None,
                norm.ctypes.data if norm is not None else None, None, None, None, out.data_ptr(),
                peaks.data_ptr() if return_peaks else None, s))
        return (out, peaks) if return_peaks else out
