#!/usr/bin/env python3
"""Generate tests/golden/spectral.npz with scipy.signal.spectrogram itself (needs scipy; nothing of the reference tree is read).
Run from the repository root:   python tools/make_golden_spectral.py

One case, the shape of the reference's per-electrode analysis (eval/suppl_fig_2.py:55-57): fs 1000, 50-sample Hann frames every
10 samples, nfft 100, power density, detrend 'constant'.  The signals are seeded (T, 18) float64 rows of which 17 columns are
channels (the 18th is there so that the row stride differs from the channel count); the trials have 50, 59, 60, 210, 220 and 380
rows (1, 1, 2, 17, 18 and 34 frames), two of them overlap.  Per trial and channel one scipy call, float64 input; the fixture holds
the signals, the ranges, scipy's frames as (sum W_i, 17, 51) and scipy's version.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, T, LD, C = 4711, 1000, 18, 17
FS, NPERSEG, NOVERLAP, NFFT = 1000, 50, 40, 100
RANGES = [(0, 50), (60, 59), (130, 60), (200, 210), (400, 220), (620, 380)]       # rows 400 .. 410 belong to two trials


def signals():
    rng = np.random.default_rng(SEED)
    t = np.arange(T)[:, None] / FS
    ch = np.arange(LD)[None, :]
    # noise on a slow drift and a channel-dependent tone: no frame is near constant, every bin carries power
    return rng.standard_normal((T, LD)) * (1.0 + 0.05 * ch) + 3.0 * np.sin(2 * np.pi * (40.0 + 7.0 * ch) * t) + 20.0 * t


def main():
    import scipy
    from scipy.signal import spectrogram
    x = signals()
    frames, counts = [], []
    for first, n in RANGES:
        per_channel = []
        for c in range(C):
            f, _, sxx = spectrogram(x[first:first + n, c], fs=FS, window="hann", nfft=NFFT, nperseg=NPERSEG, noverlap=NOVERLAP)
            per_channel.append(sxx.T)                                               # (W, 51)
        frames.append(np.stack(per_channel, axis=1))                                # (W, C, 51)
        counts.append(frames[-1].shape[0])
    out = {
        "scipy_version": np.array(scipy.__version__),
        "seed": np.array([SEED, T, LD, C], dtype=np.int64),
        "params": np.array([FS, NPERSEG, NOVERLAP, NFFT], dtype=np.int64),
        "signals": x,
        "ranges": np.array(RANGES, dtype=np.int64),
        "frame_counts": np.array(counts, dtype=np.int64),
        "frequencies": f,
        "sxx": np.concatenate(frames),
    }
    assert counts == [1, 1, 2, 17, 18, 34], counts
    path = os.path.join(ROOT, "tests", "golden", "spectral.npz")
    np.savez_compressed(path, **out)
    print("spectral: scipy", scipy.__version__, "frames per trial", counts, "sxx", out["sxx"].shape, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
