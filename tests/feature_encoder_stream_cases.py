"""The case table of the stream form of the LPC feature encoder (Part 18): signals from the generators of
tests/feature_encoder_cases.py and chunkings in frames per push.  The longest signal is 40 frames.

What every test demands is exact: the method is causal (frame i reads samples up to 160 i + 159), so any chunking of a stream
gives the bits of the whole signal as one trial.
"""
from __future__ import annotations

import numpy as np

import feature_encoder_cases as K

FRAME = K.FRAME


def signals():
    """(name, int16 signal of whole frames)."""
    return [
        ("forty", np.concatenate([K.pulses(121, FRAME * 20, 9), K.white(FRAME * 7, 10, 500.0), K.ar2(FRAME * 13, 11)])),
        ("zeros_then_speech", K.zeros_then_speech(FRAME * 14, 32, FRAME * 5 + 37)),
        ("square", K.square(FRAME * 8)),
        ("zeros", K.zeros(FRAME * 6)),
        ("white35", K.white(FRAME * 35, 15)),            # runs past two tiles
    ]


def _cycle(pattern, n_frames):
    """The pattern repeated until n_frames are used up; the last push takes what is left.  Zeros stay as pushes of nothing."""
    out, left, k = [], n_frames, 0
    while left > 0:
        c = min(pattern[k % len(pattern)], left)
        out.append(c)
        left -= c
        k += 1
    return out


CHUNKINGS = ("ones", "fours", "sixteens", "seventeen_one_fifteen", "zero_three_zero_five", "whole")


def chunking(name: str, n_frames: int):
    """Frames per push, summing to n_frames."""
    pattern = {"ones": [1], "fours": [4], "sixteens": [16], "seventeen_one_fifteen": [17, 1, 15],
               "zero_three_zero_five": [0, 3, 0, 5], "whole": [n_frames]}[name]
    out = _cycle(pattern, n_frames)
    assert sum(out) == n_frames and all(c >= 0 for c in out)
    return out


def prefix_lengths(n_frames: int):
    """Frame counts at which the reference's prefix property is checked: the borders every chunking above makes."""
    ks = set()
    for name in CHUNKINGS:
        if name == "ones":
            continue
        ks.update(np.cumsum(chunking(name, n_frames)).tolist())
    ks.update([1, 2, 3, 4, 5, 16, 17, 33, 39])
    return sorted(k for k in ks if 1 <= k < n_frames)
