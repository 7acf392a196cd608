"""Seeded synthetic inputs of the shapes BASELINE.json / SURVEY.md section 8(d) name.

No clinical data or trained weights exist offline, so every test, golden fixture and bench line uses
these generators (numpy ``default_rng``; the same numpy build runs here and on the GPU box).
"""
from __future__ import annotations

import numpy as np

from .lpcnet_weights import synthetic_features  # noqa: F401  (config 1/2/4 input)


def synthetic_ecog(seed: int, n_samples: int = 1040, n_channels: int = 64, fs: int = 1000) -> np.ndarray:
    """Config 3 input: float64 (n_samples, n_channels) ~ N(0, 50^2) uV-scale noise plus 60/120 Hz line
    components (amplitude 20) that exercise the 118-122 Hz band-stop."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_samples, dtype=np.float64)[:, None] / fs
    phase = rng.uniform(0, 2 * np.pi, size=(2, n_channels))
    x = rng.standard_normal((n_samples, n_channels)) * 50.0
    x += 20.0 * np.sin(2 * np.pi * 60.0 * t + phase[0])
    x += 20.0 * np.sin(2 * np.pi * 120.0 * t + phase[1])
    return np.ascontiguousarray(x)


def synthetic_speech_audio(seed: int, n_samples: int, fs: int = 16000) -> np.ndarray:
    """Seeded int16 stand-in for a session's microphone track: low room noise (about 12 LSB rms) plus, roughly every 1.2 s, a
    burst of 0.25 - 0.7 s of harmonics of an 90 - 220 Hz fundamental under a raised-cosine envelope, so that an energy
    based detector meets both classes of frame."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n_samples) * 12.0
    t = 0
    while True:
        t += int(rng.uniform(0.5, 1.9) * fs)
        dur = int(rng.uniform(0.25, 0.7) * fs)
        if t + dur >= n_samples:
            break
        f0 = rng.uniform(90.0, 220.0)
        k = np.arange(dur, dtype=np.float64)
        burst = np.zeros(dur)
        for h in range(1, 9):
            burst += (rng.uniform(0.3, 1.0) / h) * np.sin(2 * np.pi * f0 * h * k / fs + rng.uniform(0, 2 * np.pi))
        x[t:t + dur] += rng.uniform(2500.0, 7000.0) * (0.5 - 0.5 * np.cos(2 * np.pi * k / (dur - 1))) * burst
        t += dur
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)
