"""Spectrograms of the trials of a recording, and the speech-locked spectral power built on them, on the GPU.

The reference's per-electrode power-spectral analysis (eval/suppl_fig_2.py:41-92) calls ``scipy.signal.spectrogram`` once per
trial and channel -- 50-sample Hann frames every 10 samples at 1 kHz, zero-padded to ``nfft = 100`` -- averages the
speech-onset-aligned frames over the trials and divides by a per-channel baseline spectrum taken from calibration trials;
eval/figure_2ab.py:30-31 needs the same operator on audio (``nperseg = 800``, hop 160, ``mode='magnitude'``).
``SpectrogramGPU`` is that operator for a whole trial list and all channels in one call (csrc/spectral.hip), with the two
reductions (``locked``, ``mean``) that make the analysis possible without ever storing the (frames, channels, bins) array;
``speech_locked_power`` is the numeric part of the script.  Plotting, ``.mat`` parsing, the experiment's trial bookkeeping and
the channel-gain multiplication stay with the caller, who hands over signals and ``(first row, length)`` ranges as for
``HgaExtractorGPU.extract_trials``.

The window is computed here, from its definition, and handed to the library as data.
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import numpy as np

from . import _lib

MODES = {"psd": 0, "magnitude": 1}


class SpecParams(C.Structure):
    """dss_spec_params of include/dss_hip.h."""
    _fields_ = [("nperseg", C.c_int), ("hop", C.c_int), ("nfft", C.c_int), ("mode", C.c_int), ("detrend", C.c_int),
                ("reserved", C.c_int), ("fs", C.c_double)]


def hann_periodic(n: int) -> np.ndarray:
    """``scipy.signal.get_window('hann', n)`` bit for bit, built the way scipy defines it: the general cosine window
    0.5 cos(0 x) + 0.5 cos(1 x) over ``linspace(-pi, pi, n + 1)``, its last point dropped (the periodic, "DFT-even" form)."""
    n = int(n)
    if n <= 1:
        return np.ones(max(n, 0))
    fac = np.linspace(-np.pi, np.pi, n + 1)
    w = np.zeros(n + 1)
    for k, a in enumerate((0.5, 0.5)):
        w += a * np.cos(k * fac)
    return w[:-1]


def trial_frames(n: int, nperseg: int, hop: int) -> int:
    """(n - nperseg) // hop + 1; DssError for a trial shorter than one window (needs no GPU)."""
    return _lib.check(_lib.load().dss_spec_trial_frames_for(int(n), int(nperseg), int(hop)))


def _trial_arrays(ranges):
    t = np.asarray(list(ranges), dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])


def check_trials(n_rows: int, ranges, nperseg: int, hop: int) -> int:
    """The argument checks of the trial-list calls on their own: total frames of ``[(first row, length)]`` in signals of
    ``n_rows`` rows; DssError with the reason otherwise (needs no GPU)."""
    first, length = _trial_arrays(ranges)
    return _lib.check(_lib.load().dss_spec_check_trials(int(n_rows), len(first), first.ctypes.data, length.ctypes.data,
                                                        int(nperseg), int(hop)))


def check_locked(ranges, onsets, pre: int, post: int, nperseg: int, hop: int) -> int:
    """The checks of ``locked`` on their own: ``pre + post``; DssError naming the trial whose onset frame lies closer than
    ``pre`` frames to its start or ``post`` frames to its end (needs no GPU)."""
    _, length = _trial_arrays(ranges)
    on = np.ascontiguousarray(onsets, dtype=np.int32).reshape(-1)
    if len(on) != len(length):
        raise ValueError("onsets must hold one frame index per trial")
    return _lib.check(_lib.load().dss_spec_check_locked(len(length), length.ctypes.data, on.ctypes.data, int(pre), int(post),
                                                        int(nperseg), int(hop)))


KINDS = {"trials": 0, "locked": 1, "mean": 2}
Geometry = collections.namedtuple("Geometry", "F CG NB nblk lds_bytes")


def geometry(nperseg: int, hop: int, nfft: int, n_channels: int, kind, mode: str = "psd", detrend="constant",
             fs: float = 1000.0) -> Geometry:
    """How ``SpectrogramGPU(fs, nperseg, nperseg - hop, nfft, ...)`` will cut the workgroups of ``trials`` (kind 'trials' or
    0), ``locked`` ('locked', 1) or ``mean`` ('mean', 2) for ``n_channels`` channels: F frames x CG channels x NB blocks of 16
    bins per workgroup, ``nblk`` blocks in all, bytes of LDS.  It is the library's own choice (``dss_spec_geometry``), not a
    copy of it; DssError for parameters the library refuses (needs no GPU)."""
    p = SpecParams(int(nperseg), int(hop), int(nfft), MODES[mode], 1 if detrend == "constant" else 0, 0, float(fs))
    out = (C.c_int * 5)()
    _lib.check(_lib.load().dss_spec_geometry(C.addressof(p), int(n_channels), int(KINDS.get(kind, kind)), C.addressof(out)))
    return Geometry(*out)


class SpectrogramGPU:
    """``scipy.signal.spectrogram(x, fs, window, nperseg, noverlap, nfft, detrend, mode=...)`` over trial lists.

    ``window``: None for the periodic Hann window, or ``nperseg`` float64 values; ``mode``: 'psd' (scipy's default,
    ``scaling='density'``) or 'magnitude'; ``detrend``: 'constant' or False.  Signals are float64 ``(T, C)`` host arrays or
    CUDA tensors whose rows may be strided (a column slice of a wider recording is read in place); a one-dimensional signal
    is one channel.  int16 or float32 host input is converted, exactly, to float64 first -- scipy itself would compute such
    input in float32, so compare against scipy on the float64 samples."""

    def __init__(self, fs: float, nperseg: int, noverlap: int, nfft=None, window=None, mode: str = "psd", detrend="constant"):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        if detrend not in ("constant", False, None):
            raise ValueError("detrend must be 'constant' or False")
        self.fs = float(fs)
        self.nperseg = int(nperseg)
        self.hop = self.nperseg - int(noverlap)
        self.nfft = self.nperseg if nfft is None else int(nfft)
        self.n_bins = self.nfft // 2 + 1
        self.mode = mode
        self.params = SpecParams(self.nperseg, self.hop, self.nfft, MODES[mode], 1 if detrend == "constant" else 0, 0, self.fs)
        _lib.check(_lib.load().dss_spec_check_params(C.addressof(self.params)))
        self.window = np.ascontiguousarray(hann_periodic(self.nperseg) if window is None else window, dtype=np.float64)
        if self.window.shape != (self.nperseg,):
            raise ValueError(f"the window must hold {self.nperseg} values")
        L = _lib.require_gpu()
        self._L = L
        self._h = L.dss_spec_create(C.addressof(self.params), self.window.ctypes.data)
        if not self._h:
            raise _lib.DssError(L.dss_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.dss_spec_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def frequencies(self) -> np.ndarray:
        return np.fft.rfftfreq(self.nfft, 1.0 / self.fs)

    def trial_frames(self, n: int) -> int:
        return trial_frames(n, self.nperseg, self.hop)

    # ---- arguments ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _host(signals):
        a = np.asarray(signals)
        if a.dtype not in (np.float64, np.float32, np.int16):
            raise ValueError("signals must be float64 (or int16 / float32, converted exactly)")
        if a.ndim == 1:
            a = a[:, None]
        if a.ndim != 2 or a.shape[1] < 1:
            raise ValueError(f"expected (T, C) signals, got {a.shape}")
        if a.dtype != np.float64:
            a = a.astype(np.float64)
        if a.strides[1] != 8 or a.strides[0] % 8 or a.strides[0] < 8 * a.shape[1]:
            a = np.ascontiguousarray(a)
        ld = a.strides[0] // 8
        return a, int(ld)

    @staticmethod
    def _dev(signals):
        import torch
        if not (signals.is_cuda and signals.dtype == torch.float64):
            raise ValueError("signals must be a CUDA float64 tensor")
        t = signals[:, None] if signals.dim() == 1 else signals
        if t.dim() != 2 or t.shape[1] < 1:
            raise ValueError(f"expected (T, C) signals, got {tuple(t.shape)}")
        if (t.shape[1] > 1 and t.stride(1) != 1) or t.stride(0) < t.shape[1]:
            t = t.contiguous()
        ld = t.stride(0)
        return t, int(ld)

    def _ranges(self, n_rows, ranges):
        first, length = _trial_arrays(ranges)
        total = _lib.check(self._L.dss_spec_check_trials(int(n_rows), len(first), first.ctypes.data, length.ctypes.data,
                                                         self.nperseg, self.hop))
        return first, length, total

    def _onsets(self, length, onsets, pre, post):
        on = np.ascontiguousarray(onsets, dtype=np.int32).reshape(-1)
        if len(on) != len(length):
            raise ValueError("onsets must hold one frame index per trial")
        _lib.check(self._L.dss_spec_check_locked(len(length), length.ctypes.data, on.ctypes.data, int(pre), int(post),
                                                 self.nperseg, self.hop))
        return on

    # ---- spectrograms -------------------------------------------------------------------------------------------------
    def trials(self, signals, ranges) -> np.ndarray:
        """``signals`` (T, C) host, ``ranges`` [(first row, length)] -> float64 (sum W_i, C, n_bins): the spectrogram frames of
        every trial, trial after trial in list order (scipy's ``Sxx`` of trial i and channel c is ``out[a:b, c].T``)."""
        a, ld = self._host(signals)
        first, length, total = self._ranges(a.shape[0], ranges)
        out = np.empty((total, a.shape[1], self.n_bins), dtype=np.float64)
        if total:
            got = _lib.check(self._L.dss_spec_trials(self._h, a.ctypes.data, a.shape[0], ld, a.shape[1], len(first),
                                                     first.ctypes.data, length.ctypes.data, out.ctypes.data))
            assert got == total
        return out

    def trials_torch(self, signals, ranges, stream=None):
        """Device-resident form: CUDA float64 (T, C) -> CUDA (sum W_i, C, n_bins); queued on the current (or the given) stream,
        no synchronisation."""
        import torch
        t, ld = self._dev(signals)
        first, length, total = self._ranges(t.shape[0], ranges)
        out = torch.empty((total, t.shape[1], self.n_bins), dtype=torch.float64, device=t.device)
        s = torch.cuda.current_stream(t.device).cuda_stream if stream is None else stream
        if total:
            got = _lib.check(self._L.dss_spec_trials_dev(self._h, t.data_ptr(), t.shape[0], ld, t.shape[1], len(first),
                                                         first.ctypes.data, length.ctypes.data, out.data_ptr(), s))
            assert got == total
        return out

    # ---- the onset-locked mean ----------------------------------------------------------------------------------------
    def locked(self, signals, ranges, onsets, pre: int, post: int) -> np.ndarray:
        """float64 (C, n_bins, pre + post): column j is the mean over the trials of frame ``onsets[i] - pre + j`` of trial i
        (``np.mean(np.stack([Sxx_i[:, o_i - pre:o_i + post]]), axis=0)`` per channel), without storing any spectrogram.  A
        trial whose onset lies closer than ``pre`` frames to its start or ``post`` frames to its end is refused."""
        a, ld = self._host(signals)
        first, length, _ = self._ranges(a.shape[0], ranges)
        on = self._onsets(length, onsets, pre, post)
        out = np.empty((a.shape[1], self.n_bins, int(pre) + int(post)), dtype=np.float64)
        _lib.check(self._L.dss_spec_locked(self._h, a.ctypes.data, a.shape[0], ld, a.shape[1], len(first), first.ctypes.data,
                                           length.ctypes.data, on.ctypes.data, int(pre), int(post), out.ctypes.data))
        return out

    def locked_torch(self, signals, ranges, onsets, pre: int, post: int, stream=None):
        """Device-resident form of ``locked``; ``onsets`` stays a host sequence."""
        import torch
        t, ld = self._dev(signals)
        first, length, _ = self._ranges(t.shape[0], ranges)
        on = self._onsets(length, onsets, pre, post)
        out = torch.empty((t.shape[1], self.n_bins, int(pre) + int(post)), dtype=torch.float64, device=t.device)
        s = torch.cuda.current_stream(t.device).cuda_stream if stream is None else stream
        _lib.check(self._L.dss_spec_locked_dev(self._h, t.data_ptr(), t.shape[0], ld, t.shape[1], len(first), first.ctypes.data,
                                               length.ctypes.data, on.ctypes.data, int(pre), int(post), out.data_ptr(), s))
        return out

    # ---- the mean spectrum --------------------------------------------------------------------------------------------
    def mean(self, signals, ranges) -> np.ndarray:
        """float64 (C, n_bins): the mean over ALL frames of all trials (``np.mean(np.concatenate(Sxx_i, axis=1), axis=-1)``
        per channel)."""
        a, ld = self._host(signals)
        first, length, _ = self._ranges(a.shape[0], ranges)
        out = np.empty((a.shape[1], self.n_bins), dtype=np.float64)
        _lib.check(self._L.dss_spec_mean(self._h, a.ctypes.data, a.shape[0], ld, a.shape[1], len(first), first.ctypes.data,
                                         length.ctypes.data, out.ctypes.data))
        return out

    def mean_torch(self, signals, ranges, stream=None):
        """Device-resident form of ``mean``."""
        import torch
        t, ld = self._dev(signals)
        first, length, _ = self._ranges(t.shape[0], ranges)
        out = torch.empty((t.shape[1], self.n_bins), dtype=torch.float64, device=t.device)
        s = torch.cuda.current_stream(t.device).cuda_stream if stream is None else stream
        _lib.check(self._L.dss_spec_mean_dev(self._h, t.data_ptr(), t.shape[0], ld, t.shape[1], len(first), first.ctypes.data,
                                             length.ctypes.data, out.data_ptr(), s))
        return out


def locked_frame_counts(fs: float = 1000, window_size: float = 0.05, pre_onset: float = 0.5, post_onset: float = 1.5):
    """suppl_fig_2.py:64-65: ``floor((t fs - window fs) / (0.01 fs)) + 5`` frames before and after the onset."""
    pre = math.floor((pre_onset * fs - window_size * fs) / (0.01 * fs)) + 5
    post = math.floor((post_onset * fs - window_size * fs) / (0.01 * fs)) + 5
    return pre, post


def speech_locked_power(cal_signals, cal_ranges, signals, ranges, onsets, fs=1000, window_size: float = 0.05,
                        nb_fft_bins: int = 100, pre_onset: float = 0.5, post_onset: float = 1.5) -> np.ndarray:
    """The numeric part of eval/suppl_fig_2.py:41-92: float32 (C, nb_fft_bins // 2 + 1, pre + post) speech-locked power in dB
    over a per-channel baseline.

    ``cal_signals`` / ``cal_ranges``: the calibration recording and its trials, whose mean spectrum over all frames is the
    baseline (cast to float32, as the script stores it); ``signals`` / ``ranges``: the recording and the trials to average
    (the script's ``[start, stop + post_onset fs)``); ``onsets``: one spectrogram frame index per trial, ``np.argmax(labels)``
    of whatever voice-activity detector the caller ran on the trial's audio (the script runs ``EnergyBasedVad`` at the
    recording's rate; its frames are the spectrogram's: 50 ms every 10 ms).  Signals are host arrays or CUDA tensors; both
    reductions run on the GPU, the division, ``10 log10`` and the float32 cast of the small result on the host.  A trial whose
    onset lies too close to either end is refused, where the script silently takes a wrong slice."""
    nperseg = int(window_size * fs)
    sp = SpectrogramGPU(fs, nperseg, int(window_size * fs - 0.01 * fs), nfft=int(nb_fft_bins))
    try:
        pre, post = locked_frame_counts(fs, window_size, pre_onset, post_onset)
        on_device = hasattr(signals, "is_cuda")
        if hasattr(cal_signals, "is_cuda"):
            baseline = sp.mean_torch(cal_signals, cal_ranges)
        else:
            baseline = sp.mean(cal_signals, cal_ranges)
        if on_device:
            power = sp.locked_torch(signals, ranges, onsets, pre, post)
        else:
            power = sp.locked(signals, ranges, onsets, pre, post)
        if hasattr(baseline, "is_cuda"):
            baseline = baseline.cpu().numpy()
        if on_device:
            power = power.cpu().numpy()
    finally:
        sp.close()
    baseline = baseline.astype(np.float32)
    return (10 * np.log10(power / baseline[:, :, None])).astype(np.float32)
