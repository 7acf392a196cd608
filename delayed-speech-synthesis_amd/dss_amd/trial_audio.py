"""The loudness step of the reference's trial audio, as data and as two host functions.

``prepare_corpus._normalize_audio`` (prepare_corpus.py:33-40) sends every non-silence trial through pydub:
``effects.normalize(segment)`` and then ``segment.apply_gain(-3.0)``.  Each is one ``audioop.mul`` over the int16 samples:
``floor(sample * factor)`` in double, clipped to int16.  The library does the two multiplications (csrc/avad_gain.h, shared by
the kernels and by ``peak_host`` / ``scale_host`` below) and never evaluates a logarithm or a power: the factor of every
possible peak is a table computed here, in Python, with the very expressions pydub's wrapper evaluates, and handed over as
data (``AcousticVadGPU.set_gain``).

pydub is not installed where this was written.  The expressions are a reading of ``pydub/effects.py::normalize``,
``AudioSegment.apply_gain / max / max_possible_amplitude`` and ``utils.db_to_float / ratio_to_db``; tests/golden/TRIAL_AUDIO.md
states that and the one check to run when pydub is at hand.  Correcting the table needs no change in the library.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib

N_PEAKS = 32769                     # peaks 0 .. 32768 of int16 audio
MAX_POSSIBLE_AMPLITUDE = 32768.0    # AudioSegment.max_possible_amplitude of 16-bit audio: 2 ** 16 / 2


def _ratio_to_db(ratio: float) -> float:
    """pydub.utils.ratio_to_db(ratio) with using_amplitude=True: ``20 * log(ratio, 10)`` -- math.log with base 10, which is
    log(ratio) / log(10), not log10."""
    return 20 * math.log(ratio, 10)


def _db_to_float(db) -> float:
    """pydub.utils.db_to_float(db) with using_amplitude=True."""
    return 10 ** (float(db) / 20)


def pydub_gain_table(headroom_db: float = 0.1) -> np.ndarray:
    """float64 (32769,): entry p is the factor ``effects.normalize(segment, headroom)`` multiplies a segment of peak p by.

    ``target = max_possible_amplitude * db_to_float(-headroom)``, ``boost = ratio_to_db(target / peak)``, and ``apply_gain(boost)``
    multiplies by ``db_to_float(boost)``.  Entry 0 is 1.0: pydub returns a silent segment as it is, and floor(x * 1.0) == x."""
    target = MAX_POSSIBLE_AMPLITUDE * _db_to_float(-headroom_db)
    table = np.empty(N_PEAKS, dtype=np.float64)
    table[0] = 1.0
    for peak in range(1, N_PEAKS):
        table[peak] = _db_to_float(_ratio_to_db(target / peak))
    return table


def post_gain(db: float = -3.0) -> float:
    """The factor of ``segment.apply_gain(db)``: prepare_corpus's normalization_factor, -3 dB."""
    return _db_to_float(db)


def _int16(x) -> np.ndarray:
    a = np.asarray(x)
    if a.dtype != np.int16 or a.ndim != 1:
        raise ValueError("samples must be a one-dimensional int16 array")
    return np.ascontiguousarray(a)


def peak_host(x) -> int:
    """max |x| of int16 samples as int, 0 .. 32768 (dss_avad_peak_host: the function the peak kernel applies; needs no GPU)."""
    a = _int16(x)
    return _lib.check(_lib.load().dss_avad_peak_host(a.ctypes.data, len(a)))


def scale_host(x, factor: float) -> np.ndarray:
    """``audioop.mul(x, 2, factor)`` on int16 samples (dss_avad_scale_host: the function the kernels apply; needs no GPU)."""
    a = _int16(x)
    out = np.empty_like(a)
    _lib.check(_lib.load().dss_avad_scale_host(a.ctypes.data, len(a), float(factor), out.ctypes.data))
    return out
