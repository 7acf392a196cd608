"""A float64 numpy restatement of the acoustic VAD labels, written from the operator's definition (frames, Hann window,
direct DFT from a cos / sin table, magnitude, mel filter bank, log, 2 * sum over the bands, threshold from the trial's mean,
vote over [i - context, i + context)).  Test code: it shares no text with the package and takes the window and the mel
matrix as arguments, so a test may hand it the fixture's own tables."""
import numpy as np


def frames_of(n, window=800, shift=160):
    return (n - window) // shift + 1


def trial_samples(audio, first, n, lead):
    """`lead` zeros, then audio[first : first + n - lead], int16."""
    return np.concatenate([np.zeros(lead, dtype=np.int16), np.asarray(audio[first:first + n - lead], dtype=np.int16)])


def log_energy(x, window_fn, mel, shift=160, chunk=512):
    """x int16 (n,) -> float64 (W,)."""
    N = len(window_fn)
    W = frames_of(len(x), N, shift)
    if W <= 0:
        raise ValueError("trial shorter than one window")
    j = np.arange(N)
    bins = np.arange(N // 2 + 1)
    idx = (bins[None, :] * j[:, None]) % N                           # (N, bins)
    ang = 2.0 * np.pi * j / N
    cos_t, sin_t = np.cos(ang)[idx], np.sin(ang)[idx]
    a = np.asarray(x, dtype=np.float64) / 2.0 ** 15
    out = np.empty(W)
    for w0 in range(0, W, chunk):
        w1 = min(W, w0 + chunk)
        fr = np.stack([a[w * shift:w * shift + N] for w in range(w0, w1)]) * window_fn[None, :]
        re, im = fr @ cos_t, fr @ sin_t
        m = np.sqrt(re * re + im * im) @ mel
        out[w0:w1] = 2.0 * np.sum(np.log(m + 1e-7), axis=1)
    return out


def vote(le, energy_threshold=4.0, energy_mean_scale=1.0, frames_context=5, proportion_threshold=0.6):
    """-> (labels bool (W,), threshold, gap): gap = smallest |log energy - threshold| of the trial."""
    W = len(le)
    thr = float(energy_threshold)
    if energy_mean_scale != 0:
        thr += energy_mean_scale * np.sum(le) / W
    above = le > thr
    labels = np.empty(W, dtype=bool)
    for i in range(W):
        lo, hi = max(i - frames_context, 0), min(i + frames_context, W)
        den = max(hi - lo, 0)
        num = int(above[lo:hi].sum()) if den else 0
        labels[i] = float(num) >= float(den) * proportion_threshold
    return labels, thr, float(np.min(np.abs(le - thr)))


def near_threshold(le, thr, frames_context, margin):
    """Frames whose vote looks at a log energy within `margin` of the threshold: bool (W,)."""
    W = len(le)
    close = np.abs(le - thr) <= margin
    out = np.zeros(W, dtype=bool)
    for i in np.nonzero(close)[0]:
        out[max(i - frames_context + 1, 0):min(i + frames_context + 1, W)] = True
    return out
