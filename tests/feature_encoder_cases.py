"""The case table of the LPC feature encoder tests: trial lists as (name, [int16 trial, ...]).

The seeds are chosen so that the reference's smallest decision margin (feature_encoder_reference.Margin: every strict
comparison of the damping and the track, every argmax gap, exact ties left out) is at least MIN_MARGIN in every case;
tests/test_cpu_feature_encoder.py asserts it, so the GPU test may demand exact lags with no case left out.  The kernel's scores
differ from the reference's by rounding of O(1) fp64 sums of 80 terms (below 1e-12), far inside that margin.
"""
from __future__ import annotations

import os
import re

import numpy as np

MIN_MARGIN = 1e-9
FRAME = 160
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tile_frames() -> int:
    """Frames per workgroup of the spectrum launch, read from the kernels' header."""
    text = open(os.path.join(ROOT, "delayed-speech-synthesis_amd", "csrc", "feature_encoder.h")).read()
    return int(re.search(r"#define\s+FENC_TILE_FRAMES\s+(\d+)", text).group(1))


def _i16(v):
    return np.clip(np.rint(v), -32767, 32767).astype(np.int16)


def pulses(period: int, n: int, seed: int, amp: float = 12000.0, noise: float = 30.0) -> np.ndarray:
    """A pulse train (every pulse a short decaying ring) with a little seeded noise: the noise keeps the margins wide."""
    rng = np.random.default_rng(seed)
    v = np.zeros(n)
    v[seed % period::period] = amp
    ring = 0.6 ** np.arange(8) * np.cos(0.9 * np.arange(8))
    return _i16(np.convolve(v, ring)[:n] + noise * rng.standard_normal(n))


def white(n: int, seed: int, sigma: float = 3000.0) -> np.ndarray:
    return _i16(sigma * np.random.default_rng(seed).standard_normal(n))


def ar2(n: int, seed: int, f: float = 1000.0, r: float = 0.97, sigma: float = 200.0) -> np.ndarray:
    """An AR(2) resonance at f Hz driven by seeded noise."""
    u = sigma * np.random.default_rng(seed).standard_normal(n)
    a1, a2 = 2 * r * np.cos(2 * np.pi * f / 16000.0), -r * r
    y = np.zeros(n)
    for t in range(n):
        y[t] = u[t] + (a1 * y[t - 1] if t > 0 else 0.0) + (a2 * y[t - 2] if t > 1 else 0.0)
    return _i16(y)


def square(n: int, period: int = 100) -> np.ndarray:
    return _i16(np.where((np.arange(n) // (period // 2)) % 2 == 0, 32767.0, -32767.0))


def zeros(n: int) -> np.ndarray:
    return np.zeros(n, np.int16)


def zeros_then_speech(n: int, seed: int, lead: int) -> np.ndarray:
    """`lead` zeros, then a pulse train through a resonance plus noise: switches the floor and the max(1, .) denominator."""
    m = n - lead
    p = pulses(117, m, seed, amp=6000.0, noise=5.0).astype(np.float64)
    y = np.zeros(m)
    for t in range(m):
        y[t] = p[t] + (1.3 * y[t - 1] if t > 0 else 0.0) - (0.6 * y[t - 2] if t > 1 else 0.0)
    return np.concatenate([zeros(lead), _i16(0.5 * y)])


# Pulse periods the track locks to from the fourth frame on, for each of PULSE_SEEDS (tests/test_cpu_feature_encoder.py asserts
# it).  Tried: 33, 34 and 100 lock; 255 and 256 do NOT (a sub-frame is 80 samples: two out of three hold no pulse, their scores
# are noise and the track leaves the lag in some frames; 256 mostly reports 255).  Every period from 100 to 167 locks, beyond
# that only scattered ones; 213 is the largest that does, so 167 and 213 stand in for the upper edge.  255 and 256 stay in the
# kernel's case table as signals.
LOCKED_PERIODS = (33, 34, 100, 167, 213)
UNLOCKED_EDGE_PERIODS = (255, 256)
PULSE_SEEDS = (20, 21, 22)


def cases():
    T = tile_frames()
    out = []
    out.append(("lengths", [white(0, 1), white(159, 2), pulses(60, 160, 3), white(161, 4), ar2(319, 5), white(320, 6),
                            pulses(80, 640, 7), white(800, 8)]))
    out.append(("long_trial", [np.concatenate([pulses(121, 16000, 9), white(16000, 10, 500.0), ar2(16000 + 77, 11)])]))
    out.append(("tile_edges", [white(FRAME * (T - 1) + 5, 12), pulses(90, FRAME * T, 13), ar2(FRAME * (T + 1) + 159, 14),
                               white(FRAME * (2 * T - 1), 15), white(FRAME * 2 * T + 1, 16), pulses(150, FRAME * (2 * T + 1), 17)]))
    out.append(("empty_between", [pulses(70, 1000, 18), zeros(0), white(1300, 19)]))
    out.append(("pulse_edges", [pulses(p, FRAME * 12, 20 + k % 3) for k, p in enumerate(LOCKED_PERIODS + UNLOCKED_EDGE_PERIODS)]))
    out.append(("signals", [white(FRAME * 8, 30), ar2(FRAME * 8, 31), square(FRAME * 8), zeros(FRAME * 6),
                            zeros_then_speech(FRAME * 14, 32, FRAME * 5 + 37)]))
    return out


def concatenate(trials):
    """(int16 concatenation, int64 offsets) as session_trial_audio returns them."""
    offs = np.concatenate([[0], np.cumsum([len(t) for t in trials])]).astype(np.int64)
    audio = np.concatenate(trials).astype(np.int16) if trials else np.zeros(0, np.int16)
    return audio, offs
