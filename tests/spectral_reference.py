"""float64 numpy restatement of scipy.signal.spectrogram (no padding, no boundary extension) with a direct DFT, and of the
reductions the reference's spectral analysis takes of it (eval/suppl_fig_2.py:41-92).  Used for what tests/golden/spectral.npz
does not hold: the onset-locked mean, the baseline, detrend off."""
import math

import numpy as np

U = 2.0 ** -53


def frames_of(n, nperseg, hop):
    return (n - nperseg) // hop + 1


def spectrogram(x, fs, window, nperseg, hop, nfft, mode="psd", detrend=True):
    """x (n, C) float64 -> (W, C, nfft // 2 + 1): frame w is rows w * hop .. w * hop + nperseg - 1."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    W = frames_of(len(x), nperseg, hop)
    seg = x[np.arange(W)[:, None] * hop + np.arange(nperseg)[None, :]]              # (W, nperseg, C)
    if detrend:
        seg = seg - seg.mean(axis=1, keepdims=True)
    seg = seg * np.asarray(window, dtype=np.float64)[None, :, None]
    bins = nfft // 2 + 1
    ang = 2.0 * np.pi * ((np.arange(bins)[:, None] * np.arange(nperseg)[None, :]) % nfft) / nfft
    re = np.einsum("bn,wnc->wcb", np.cos(ang), seg)
    im = np.einsum("bn,wnc->wcb", np.sin(ang), seg)
    scale = 1.0 / (fs * (window * window).sum())
    if mode == "magnitude":
        return np.sqrt(re * re + im * im) * np.sqrt(scale)
    p = (re * re + im * im) * scale
    if nfft % 2:
        p[..., 1:] *= 2
    else:
        p[..., 1:-1] *= 2
    return p


def frame_bound(values, nperseg, mode="psd"):
    """The issue's bound per frame and channel, broadcast over the bins: 2 (n + 8) sqrt(n) 2^-53 of the frame's largest bin
    for the power density, half that factor for the magnitude.  values (..., bins) -> (..., 1)."""
    factor = 2.0 * (nperseg + 8) * math.sqrt(nperseg) * U
    if mode == "magnitude":
        factor *= 0.5
    return factor * np.max(values, axis=-1, keepdims=True)


def trials(x, ranges, fs, window, nperseg, hop, nfft, mode="psd", detrend=True):
    return np.concatenate([spectrogram(x[a:a + n], fs, window, nperseg, hop, nfft, mode, detrend) for a, n in ranges])


def locked(x, ranges, onsets, pre, post, fs, window, nperseg, hop, nfft, mode="psd", detrend=True):
    """((C, bins, pre + post) mean, the same shape of bounds): the mean over the trials of frames onset - pre .. onset + post."""
    cut = [spectrogram(x[a:a + n], fs, window, nperseg, hop, nfft, mode, detrend)[o - pre:o + post] for (a, n), o in zip(ranges, onsets)]
    assert all(len(c) == pre + post for c in cut)
    mean = np.mean(np.stack(cut), axis=0)                                           # (J, C, bins)
    bound = np.mean(np.stack([np.broadcast_to(frame_bound(c, nperseg, mode), c.shape) for c in cut]), axis=0) + len(cut) * U * np.abs(mean)
    return mean.transpose(1, 2, 0), bound.transpose(1, 2, 0)


def mean(x, ranges, fs, window, nperseg, hop, nfft, mode="psd", detrend=True):
    """((C, bins) mean over all frames of all trials, bounds)."""
    s = trials(x, ranges, fs, window, nperseg, hop, nfft, mode, detrend)            # (frames, C, bins)
    m = np.mean(s, axis=0)
    return m, np.mean(np.broadcast_to(frame_bound(s, nperseg, mode), s.shape), axis=0) + len(s) * U * np.abs(m)


def speech_locked_power(cal, cal_ranges, x, ranges, onsets, fs=1000, window_size=0.05, nb_fft_bins=100, pre_onset=0.5, post_onset=1.5):
    """suppl_fig_2.py:41-92 line by line on arrays: (float32 (C, bins, pre + post) dB, the float64 ratio mean / baseline)."""
    from dss_amd.spectral import hann_periodic
    nperseg = int(window_size * fs)
    hop = nperseg - int(window_size * fs - 0.01 * fs)
    window = hann_periodic(nperseg)
    C, bins = cal.shape[1], int(nb_fft_bins // 2) + 1
    normalization_statistics = np.zeros((C, bins), dtype=np.float32)
    base = trials(cal, cal_ranges, fs, window, nperseg, hop, nb_fft_bins)
    for channel in range(C):
        normalization_statistics[channel] = np.mean(base[:, channel, :].T, axis=-1)
    num_windows = math.floor((pre_onset * fs + post_onset * fs - (window_size * fs)) / (0.01 * fs)) + 5
    pre = math.floor((pre_onset * fs - (window_size * fs)) / (0.01 * fs)) + 5
    post = math.floor((post_onset * fs - (window_size * fs)) / (0.01 * fs)) + 5
    assert num_windows == pre + post
    out = np.zeros((C, bins, num_windows), dtype=np.float32)
    ratio = np.zeros((C, bins, num_windows))
    spec = [spectrogram(x[a:a + n], fs, window, nperseg, hop, nb_fft_bins) for a, n in ranges]
    for channel in range(C):
        cut = [s[o - pre:o + post, channel, :].T for s, o in zip(spec, onsets)]
        channel_spectrogram = np.mean(np.stack(cut), axis=0)
        baseline = np.tile(normalization_statistics[channel], (channel_spectrogram.shape[1], 1)).T
        ratio[channel] = channel_spectrogram / baseline
        out[channel, :, :] = 10 * np.log10(channel_spectrogram / baseline)
    return out, ratio
