"""The acoustic contamination analysis: does the microphone signal leak into the ECoG channels in the band the decoder reads?

Stage 1 of the reference's ``replicate.sh`` (eval/contamination/run_contamination_analysis.m) drives a MATLAB toolbox after
Roussel et al. that the reference does not ship; the Python around it only prepares ``.mat`` files
(eval/contamination/aggregate_per_day.py) and plots three numbers per day (gen_contamination_report.py).  This module computes
those numbers.  The parameters are the driver script's; everything else is this project's own statement of the published method
(tests/contamination_reference.py), so parity with the toolbox's output is NOT pinned -- but a Pearson correlation
does not change under positive scaling of either side, so the toolbox's spectrogram normalisation cannot matter.

Per day: magnitude spectrograms (symmetric Hamming window of ``window`` seconds, ``spg_fs`` frames per second, the bins inside
``band``) of the audio and of every channel; for every lag of up to ``max_lag`` seconds, channel, audio bin and neural bin the
Pearson correlation over the kept frames; the contamination matrix (lag 0, the maximum over the channels); its mean diagonal
against the mean "diagonal" of column-permuted copies.  The correlation sums are the hot path and run on the GPU
(csrc/contamination.hip, Part 12 of include/dss_hip.h) without ever storing a channel's spectrogram; artifact detection, the
matrix and the permutations are small and stay numpy.  ``.mat`` I/O and plotting stay with the caller.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib

U = 2.0 ** -53

Moments = collections.namedtuple("Moments", "n shift sa saa sb sbb sab")
Analysis = collections.namedtuple("Analysis", "surrogate_measures dataset_measure criterion_value matrix correlations")
Plan = collections.namedtuple("Plan", "frames tiles chunks tiles_per_chunk lag_groups lags_per_wave")


class ContamParams(C.Structure):
    """dss_contam_params of include/dss_hip.h."""
    _fields_ = [("nperseg", C.c_int), ("hop", C.c_int), ("bin_lo", C.c_int), ("n_bins", C.c_int), ("max_lag", C.c_int),
                ("reserved", C.c_int)]


def hamming_symmetric(n: int) -> np.ndarray:
    """0.54 - 0.46 cos(2 pi k / (n - 1)), as ``scipy.signal.get_window('hamming', n, fftbins=False)`` builds it, bit for bit:
    the general cosine window 0.54 cos(0 x) + 0.46 cos(1 x) over ``linspace(-pi, pi, n)``."""
    n = int(n)
    if n <= 1:
        return np.ones(max(n, 0))
    fac = np.linspace(-np.pi, np.pi, n)
    w = np.zeros(n)
    for k, a in enumerate((0.54, 1.0 - 0.54)):                                # scipy: general_cosine(n, [alpha, 1. - alpha])
        w += a * np.cos(k * fac)
    return w


def kept_bins(fs: float, nperseg: int, band) -> np.ndarray:
    """The one-sided DFT bins k with ``band[0] <= k fs / nperseg <= band[1]``, the frequency computed exactly so (not as
    ``k / (nperseg / fs)``, which can round a band edge that lies on a bin to the other side)."""
    f = np.arange(int(nperseg) // 2 + 1) * float(fs) / int(nperseg)
    return np.where((f >= band[0]) & (f <= band[1]))[0]


def frames_for(n_rows: int, nperseg: int, hop: int, max_lag: int = 0) -> int:
    """(n_rows - nperseg) // hop + 1; DssError for a recording shorter than one window (needs no GPU)."""
    return _lib.check(_lib.load().dss_contam_frames_for(int(n_rows), int(nperseg), int(hop), int(max_lag)))


def launch_plan(params: ContamParams, n_rows: int, n_channels: int) -> Plan:
    """How the library cuts a call into workgroups (``dss_contam_plan``; needs no GPU): frames, tiles of 32 frames, chunks of
    ``tiles_per_chunk`` tiles (the last may hold fewer), lag groups of the grid, lags per wave."""
    plan = (C.c_int * 6)()
    _lib.check(_lib.load().dss_contam_plan(C.addressof(params), int(n_rows), int(n_channels), C.addressof(plan)))
    return Plan(*plan)


def frame_mask(keep, nperseg: int, hop: int) -> np.ndarray:
    """Per-sample boolean ``keep`` -> per-frame: frame t is kept iff every sample in [t hop, t hop + nperseg) is kept."""
    keep = np.asarray(keep, dtype=bool).reshape(-1)
    W = (len(keep) - nperseg) // hop + 1
    if W < 1:
        return np.zeros(0, dtype=bool)
    dropped = np.concatenate([[0], np.cumsum(~keep)])
    start = np.arange(W) * hop
    return dropped[start + nperseg] == dropped[start]


def speech_periods(labels, frame_s: float = 0.01) -> np.ndarray:
    """aggregate_per_day.py:60-66: the changes of 10 ms VAD labels as float32 (k, 2) ``(start, stop)`` seconds, ``stop`` one
    frame early as the script has it.  Labels that start inside speech, or end inside it, are the script's to misread; a
    trailing unpaired change is dropped."""
    labels = np.asarray(labels).reshape(-1)
    diff = np.where(labels[:-1] != labels[1:])[0] + 1
    diff = diff.astype(np.float32)
    diff[1::2] -= 1
    diff *= np.float32(frame_s)
    k = len(diff) // 2
    timings = np.zeros(shape=(k, 2), dtype=np.float32)
    timings[:, 0] = diff[0::2][:k]
    timings[:, 1] = diff[1::2][:k]
    return timings


def periods_mask(periods, n_rows: int, fs: float) -> np.ndarray:
    """Boolean (n_rows,): samples inside any ``(start, stop)`` seconds period, both ends included."""
    m = np.zeros(int(n_rows), dtype=bool)
    for a, b in np.asarray(periods, dtype=np.float64).reshape(-1, 2):
        lo, hi = max(0, int(round(a * fs))), min(int(n_rows), int(round(b * fs)) + 1)
        if hi > lo:
            m[lo:hi] = True
    return m


def detect_artifacts(brain, fs: float, span: float = 0.5, factor: float = 5.0, ratio: float = 0.1, safety: float = 0.5) -> np.ndarray:
    """Boolean (T,) artifact samples of float64 (T, C) ``brain``.  Every channel less its centred moving average over
    ``round(span fs)`` samples (made odd by dropping one; a cumulative sum, the window shrinking at the ends), less the median
    of that: ``d``.  A channel crosses at a sample where ``|d| > factor median(|d|)``; a sample is an artifact where at least
    ``ratio C`` channels cross; artifacts are widened by ``round(safety fs)`` samples to both sides."""
    x = np.asarray(brain, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    T, Cn = x.shape
    m = max(1, int(round(span * fs)))
    half = (m - 1) // 2
    lo = np.maximum(np.arange(T) - half, 0)
    hi = np.minimum(np.arange(T) + half + 1, T)
    cs = np.concatenate([np.zeros((1, Cn)), np.cumsum(x, axis=0)])
    d = x - (cs[hi] - cs[lo]) / (hi - lo)[:, None]
    d = d - np.median(d, axis=0)
    crossing = np.abs(d) > factor * np.median(np.abs(d), axis=0)
    art = crossing.sum(axis=1) >= ratio * Cn
    w = int(round(safety * fs))
    if w > 0 and art.any():
        c = np.concatenate([[0], np.cumsum(art)])
        art = c[np.minimum(np.arange(T) + w + 1, T)] - c[np.maximum(np.arange(T) - w, 0)] > 0
    return art


def correlations_from_moments(m: Moments) -> np.ndarray:
    """(lags, C, B, B) Pearson correlations from the sums: (sab - sa sb / n) / sqrt((saa - sa^2 / n) (sbb - sb^2 / n)); NaN
    with fewer than two frames or zero variance on either side.  A variance counts as zero when it is at most
    4 n 2^-53 of the sum of squares, the size of the sums' own rounding."""
    with np.errstate(divide="ignore", invalid="ignore"):
        n = m.n[:, None]
        va = m.saa - m.sa * m.sa / n                                                  # (lags, B)
        ok_a = (n >= 2) & (va > 4 * n * U * m.saa)
        nc = m.n[:, None, None]
        vb = m.sbb - m.sb * m.sb / nc                                                 # (lags, C, B)
        ok_b = (nc >= 2) & (vb > 4 * nc * U * m.sbb)
        cov = m.sab - m.sa[:, None, :, None] * m.sb[:, :, None, :] / m.n[:, None, None, None]
        r = cov / np.sqrt(va[:, None, :, None] * vb[:, :, None, :])
    r[~(ok_a[:, None, :, None] & ok_b[:, :, None, :])] = np.nan
    return r


def contamination_matrix(r0) -> np.ndarray:
    """(C, B, B) lag-0 correlations -> (B, B): the maximum over the channels, NaN entries skipped (NaN where every channel's is)."""
    r0 = np.asarray(r0, dtype=np.float64)
    out = np.full(r0.shape[1:], np.nan)
    some = ~np.all(np.isnan(r0), axis=0)
    out[some] = np.nanmax(r0[:, some], axis=0)
    return out


def statistical_criterion(M, n_surrogates: int = 10000, seed: int = 0):
    """``(surrogate_measures float32 (S,), dataset_measure, criterion_value)``, what the reference's ``out`` struct holds:
    the mean diagonal of M, the means ``mean_i M[i, perm_s(i)]`` over S permutations of the columns drawn from
    ``numpy.random.Generator(PCG64(seed))``, and the share of surrogates that reach the dataset's measure.  A NaN on the
    diagonal of M (a bin that is constant in the audio or in every channel) leaves no measure to compare: the measure and the
    criterion value are then both NaN, never a 0 that would read as "contaminated"."""
    M = np.asarray(M, dtype=np.float64)
    B = M.shape[0]
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = np.arange(B)
    sur = np.empty(int(n_surrogates))
    for s in range(int(n_surrogates)):
        sur[s] = np.mean(M[rows, rng.permutation(B)])
    measure = float(np.mean(np.diag(M)))
    if np.isnan(measure):
        return sur.astype(np.float32), measure, float("nan")
    return sur.astype(np.float32), measure, float(np.count_nonzero(sur >= measure)) / len(sur)


class ContaminationGPU:
    """The lagged audio-ECoG spectrogram correlations of one recording day on the GPU.

    ``nperseg = round(window fs)``, ``hop = round(fs / spg_fs)``, the bins with ``band[0] <= k fs / nperseg <= band[1]``, lags
    of up to ``round(max_lag spg_fs)`` frames to both sides.  ``brain`` is float64 (T, C), host array or CUDA tensor, whose rows
    may be strided (a column slice of a wider recording is read in place); ``audio`` float64 (T,) at the same rate; ``keep`` an
    optional boolean per-sample mask."""

    def __init__(self, fs: float, window: float = 0.2, spg_fs: float = 50, band=(70, 170), max_lag: float = 0.5):
        self.fs = float(fs)
        self.nperseg = int(round(window * fs))
        self.hop = int(round(fs / spg_fs))
        self.max_lag = int(round(max_lag * spg_fs))
        inside = kept_bins(self.fs, self.nperseg, band) if self.nperseg >= 2 else np.zeros(0, dtype=np.intp)
        self.bin_lo = int(inside[0]) if len(inside) else 0
        self.n_bins = len(inside)
        self.params = ContamParams(self.nperseg, self.hop, self.bin_lo, self.n_bins, self.max_lag, 0)
        _lib.check(_lib.load().dss_contam_check_params(C.addressof(self.params)))
        self._freqs = inside * self.fs / self.nperseg
        self.window = np.ascontiguousarray(hamming_symmetric(self.nperseg))
        L = _lib.require_gpu()
        self._L = L
        self._h = L.dss_contam_create(C.addressof(self.params), self.window.ctypes.data)
        if not self._h:
            raise _lib.DssError(L.dss_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.dss_contam_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def frequencies(self) -> np.ndarray:
        return self._freqs

    @property
    def lags(self) -> np.ndarray:
        return np.arange(-self.max_lag, self.max_lag + 1)

    def frames(self, n_rows: int) -> int:
        return frames_for(n_rows, self.nperseg, self.hop, self.max_lag)

    def plan(self, n_rows: int, n_channels: int) -> Plan:
        """The launch plan of a call on ``n_rows`` rows of ``n_channels`` channels (``launch_plan``)."""
        return launch_plan(self.params, n_rows, n_channels)

    # ---- arguments ----------------------------------------------------------------------------------------------------
    def _layout(self, n_channels):
        off = (C.c_longlong * 7)()
        total = _lib.check(self._L.dss_contam_result_size(C.addressof(self.params), int(n_channels), C.addressof(off)))
        return list(off) + [total]

    def _keep_frames(self, keep, n_rows):
        if keep is None:
            return None
        keep = np.asarray(keep, dtype=bool).reshape(-1)
        if len(keep) != n_rows:
            raise ValueError(f"keep must hold one value per sample ({n_rows}), not {len(keep)}")
        return np.ascontiguousarray(frame_mask(keep, self.nperseg, self.hop), dtype=np.uint8)

    def _split(self, flat, n_channels, off) -> Moments:
        nl, B = 2 * self.max_lag + 1, self.n_bins
        shapes = [(nl,), (B,), (nl, B), (nl, B), (nl, n_channels, B), (nl, n_channels, B), (nl, n_channels, B, B)]
        return Moments(*[flat[off[k]:off[k + 1]].reshape(shapes[k]) for k in range(7)])

    # ---- the sums -----------------------------------------------------------------------------------------------------
    def moments(self, brain, audio, keep=None) -> Moments:
        """Host arrays -> ``Moments(n, shift, sa, saa, sb, sbb, sab)`` (Part 12 of include/dss_hip.h): per lag the number of
        frame pairs, the sums of the audio's magnitudes less ``shift`` and of their squares (lags, B), of the channels'
        magnitudes and of their squares (lags, C, B), and of the products (lags, C, B audio, B neural)."""
        from .spectral import SpectrogramGPU
        a, ld = SpectrogramGPU._host(brain)
        au = np.ascontiguousarray(audio, dtype=np.float64).reshape(-1)
        if len(au) != a.shape[0]:
            raise ValueError(f"audio holds {len(au)} samples, the brain signals {a.shape[0]} rows")
        self.frames(a.shape[0])
        kf = self._keep_frames(keep, a.shape[0])
        off = self._layout(a.shape[1])
        flat = np.empty(off[7], dtype=np.float64)
        _lib.check(self._L.dss_contam_moments(self._h, a.ctypes.data, a.shape[0], ld, a.shape[1], au.ctypes.data,
                                              None if kf is None else kf.ctypes.data, flat.ctypes.data))
        return self._split(flat, a.shape[1], off)

    def moments_torch(self, brain, audio, keep=None, stream=None) -> Moments:
        """Device-resident form: CUDA float64 tensors in, CUDA tensors out; queued on the current (or the given) stream, no
        synchronisation.  ``keep`` stays a host array."""
        import torch
        from .spectral import SpectrogramGPU
        t, ld = SpectrogramGPU._dev(brain)
        if not (audio.is_cuda and audio.dtype == torch.float64):
            raise ValueError("audio must be a CUDA float64 tensor")
        au = audio.reshape(-1).contiguous()
        if au.shape[0] != t.shape[0]:
            raise ValueError(f"audio holds {au.shape[0]} samples, the brain signals {t.shape[0]} rows")
        self.frames(t.shape[0])
        kf = self._keep_frames(keep, t.shape[0])
        off = self._layout(t.shape[1])
        flat = torch.empty(off[7], dtype=torch.float64, device=t.device)
        s = torch.cuda.current_stream(t.device).cuda_stream if stream is None else stream
        _lib.check(self._L.dss_contam_moments_dev(self._h, t.data_ptr(), t.shape[0], ld, t.shape[1], au.data_ptr(),
                                                  None if kf is None else kf.ctypes.data, flat.data_ptr(), s))
        return self._split(flat, t.shape[1], off)

    def correlations(self, brain, audio, keep=None) -> np.ndarray:
        """float64 (2 L + 1, C, B, B): ``r[l + L, c, i, j]`` is the Pearson correlation of audio bin i at frame t + l with bin j
        of channel c at frame t, over the frames where both are inside the recording and kept; NaN where undefined."""
        if hasattr(brain, "is_cuda"):
            m = Moments(*[v.cpu().numpy() for v in self.moments_torch(brain, audio, keep)])
        else:
            m = self.moments(brain, audio, keep)
        return correlations_from_moments(m)


def contamination_analysis(brain, audio, fs: float, window: float = 0.2, spg_fs: float = 50, band=(70, 170), max_lag: float = 0.5,
                           select_periods=None, exclude_periods=None, artifacts=(0.5, 5.0, 0.1, 0.5), n_surrogates: int = 10000,
                           seed: int = 0) -> Analysis:
    """The whole stage for one day, with the driver script's parameters as defaults: ``Analysis(surrogate_measures,
    dataset_measure, criterion_value, matrix, correlations)``.  ``select_periods`` / ``exclude_periods``: (k, 2) seconds, as
    ``speech_periods`` gives them (the script passes none); ``artifacts``: (span s, threshold factor, channel ratio, safety s)
    or None to skip the detection.  ``brain`` and ``audio`` are host arrays or CUDA tensors; the detection reads a host copy."""
    n_rows = brain.shape[0]
    keep = np.ones(n_rows, dtype=bool)
    if select_periods is not None and len(select_periods):
        keep &= periods_mask(select_periods, n_rows, fs)
    if exclude_periods is not None and len(exclude_periods):
        keep &= ~periods_mask(exclude_periods, n_rows, fs)
    if artifacts is not None:
        host = brain.cpu().numpy() if hasattr(brain, "is_cuda") else brain
        keep &= ~detect_artifacts(host, fs, *artifacts)
    op = ContaminationGPU(fs, window, spg_fs, band, max_lag)
    try:
        r = op.correlations(brain, audio, None if keep.all() else keep)
    finally:
        op.close()
    M = contamination_matrix(r[op.max_lag])
    sur, measure, p = statistical_criterion(M, n_surrogates, seed)
    return Analysis(sur, measure, p, M, r)
