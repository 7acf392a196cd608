"""Shapes of the spectrogram kernels (csrc/spectral.hip) for the tests (helper module, no tests in it).

A call's workgroups are cut at run time into F frames x CG channels x NB blocks of 16 bins (``dss_spec_pick_geom``), and every
index expression of the three kernels depends on the cut.  ``CASES`` is the list of parameters that, together, reach every F
below 32 in all three kernels, a last group of bin blocks that is not full, several channel groups beside it, and CG = 8 with
a partial group.  Which cut a case really gets is NOT taken from here: tests/test_cpu_spectral.py asks the library
(``dss_amd.spectral.geometry``) and proves the coverage, tests/test_gpu_spectral.py asserts ``EXPECTED_F`` before it runs a
case, and both take parameters, signals, trials and onsets from this module so that they cannot drift apart.  Everything is
seeded and generated, nothing is stored.
"""
from __future__ import annotations

import numpy as np

FS = 1000.0
KINDS = ("trials", "locked", "mean")

# (name, nperseg, hop, nfft, C, mode, detrend)
CASES = (
    ("n300", 300, 300, 300, 3, "psd", True),
    ("n640", 640, 640, 640, 5, "psd", True),
    ("n1000", 1000, 1000, 1000, 3, "psd", False),
    ("n1500mag", 1500, 1500, 1500, 2, "magnitude", True),
    ("n2048", 2048, 2048, 2048, 2, "psd", True),
    ("n2047", 2047, 2047, 2047, 2, "psd", True),
    ("n1024h256", 1024, 256, 2048, 3, "psd", True),
    ("wide1100", 50, 10, 1100, 17, "psd", True),
    ("cg8", 50, 10, 1000, 5, "psd", True),
    ("n128", 128, 32, 1500, 6, "psd", True),
    ("n2", 2, 1, 2, 3, "psd", True),
    ("n3odd", 3, 2, 5, 3, "psd", True),
    ("hop51", 50, 51, 64, 3, "psd", True),
    ("hopfar", 50, 10**6, 100, 3, "psd", True),
)
NAMES = tuple(c[0] for c in CASES)

# F of (trials, locked, mean) that a case is there to reach
EXPECTED_F = {"n300": (16, 16, 16), "n640": (8, 8, 8), "n1000": (4, 4, 4), "n1500mag": (2, 2, 2), "n2048": (1, 1, 1),
              "n2047": (2, 1, 1), "n1024h256": (16, 8, 8), "wide1100": (32, 32, 32), "cg8": (32, 32, 32), "n128": (32, 32, 32),
              "n2": (32, 32, 32), "n3odd": (32, 32, 32), "hop51": (32, 32, 32), "hopfar": (32, 32, 32)}

# Frames per trial, in list order (not by length: the library sorts its descriptor tables itself).  For the case's largest F:
# one trial has fewer frames (where F > 1), one has more than F and no multiple of it, so that several tiles run and the last
# one is partial.  hopfar's trials have one frame each: a second frame would start a million rows on.
_FRAMES = {32: (7, 41, 35), 16: (9, 37, 21), 8: (5, 19, 12), 4: (3, 11, 6), 2: (1, 5, 3), 1: (1, 3, 2)}
# The onset-locked mean: (trial indices, onset frames, pre, post).  The list repeats a trial and leaves the order of the trial
# list; pre + post is no multiple of F.  At F = 32 and F = 4 it lies below F and every trial takes part; elsewhere it lies
# above F, several column ranges run, and the shortest trial cannot take part.
_LOCKED = {32: ((2, 0, 1, 2), (4, 2, 30, 17), 2, 3), 16: ((2, 1, 2), (18, 20, 17), 17, 3), 8: ((1, 2, 1), (4, 3, 8), 3, 8),
           4: ((2, 0, 1, 2), (1, 1, 7, 4), 1, 2), 2: ((1, 2, 1), (1, 0, 2), 0, 3), 1: ((1, 2, 1), (1, 0, 0), 0, 2)}
_LOCKED_WIDE = ((2, 1, 2), (2, 5, 1), 1, 33)       # F 32 with pre + post = 34: two column ranges, the second with 2 live frames


def params(name):
    return CASES[NAMES.index(name)]


def frames_per_trial(name):
    if name == "hopfar":
        return (1, 1, 1)
    if name == "n1024h256":
        return (5, 37, 21)                           # its F differs by kernel: the shortest trial lies below the smaller one too
    return _FRAMES[max(EXPECTED_F[name])]


def ranges(name):
    """[(first row, length)]: the trials overlap, and (where the hop allows) none ends on its last frame's last row."""
    _, nperseg, hop, _, _, _, _ = params(name)
    out, first = [], 3
    for k, w in enumerate(frames_per_trial(name)):
        rem = (23, 73, 120)[k] if name == "hopfar" else ((k + 1) * (hop - 1)) // 4
        length = (w - 1) * hop + nperseg + rem
        out.append((first, length))
        first += length // 2 + 1 + k
    return out


def locked(name):
    """(ranges of the trials to average, onset frames, pre, post)."""
    if name == "hopfar":
        idx, onsets, pre, post = (2, 0, 1, 2), (0, 0, 0, 0), 0, 1
    elif name in ("wide1100", "hop51"):
        idx, onsets, pre, post = _LOCKED_WIDE
    else:
        idx, onsets, pre, post = _LOCKED[max(EXPECTED_F[name])]
    r = ranges(name)
    return [r[i] for i in idx], list(onsets), pre, post


def signals(name):
    """float64 (rows, C), read-only: per channel noise of scale 1 + c, an offset of 0.5 and a slow linear drift, so that
    detrending matters and no frame is nearly silent."""
    k = NAMES.index(name)
    C = CASES[k][4]
    rows = max(a + n for a, n in ranges(name)) + 5
    rng = np.random.default_rng(9100 + k)
    c = np.arange(C)[None, :]
    x = rng.standard_normal((rows, C)) * (1.0 + c) + 0.5 + 2e-4 * (1.0 + c) * np.arange(rows)[:, None]
    x.setflags(write=False)
    return x


def scipy_trials(name, x=None):
    """scipy.signal.spectrogram per trial and channel: (sum W, C, bins) in the layout of ``SpectrogramGPU.trials``.  Frames
    that do not overlap (hop > nperseg) are handed to scipy one by one: it sees rows w hop .. w hop + nperseg of the trial."""
    from scipy.signal import spectrogram
    _, nperseg, hop, nfft, C, mode, detrend = params(name)
    x = signals(name) if x is None else x
    kw = dict(fs=FS, window="hann", nperseg=nperseg, nfft=nfft, mode=mode, detrend="constant" if detrend else False)
    out = []
    for a, n in ranges(name):
        if hop > nperseg:
            starts = [a + w * hop for w in range((n - nperseg) // hop + 1)]
            per = [np.concatenate([spectrogram(x[s:s + nperseg, c], noverlap=0, **kw)[2].T for s in starts]) for c in range(C)]
        else:
            per = [spectrogram(x[a:a + n, c], noverlap=nperseg - hop, **kw)[2].T for c in range(C)]
        out.append(np.stack(per, axis=1))
    return np.concatenate(out)
