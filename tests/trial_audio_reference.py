"""A numpy restatement of the trial audio as the reference prepares it (prepare_corpus.py:33-40, 58-69): the peak of the cut,
pydub's two gains as two ``audioop.mul`` (floor of the double product, clipped as audioop's fbound clips), the 16 ms shift.
Test code: it shares no text with the package.  tests/test_cpu_trial_audio.py holds ``scale`` to Python's own ``audioop.mul``
on every int16 value."""
import hashlib
import math

import numpy as np


def peak(x):
    """max |x| as int; -32768 counts as 32768; 0 for no samples."""
    x = np.asarray(x, dtype=np.int16)
    return int(np.max(np.abs(x.astype(np.int32)))) if len(x) else 0


def scale(x, factor):
    """audioop.mul(x, 2, factor): floor(x * factor) in float64, above 32767 -> 32767, below -32767 -> -32768."""
    v = np.asarray(x, dtype=np.int16).astype(np.float64) * np.float64(factor)
    v = np.where(v > 32767.0, 32767.0, np.where(v < -32767.0, -32768.0, v))
    return np.floor(v).astype(np.int16)


def gain_table(headroom_db=0.1):
    """pydub's effects.normalize factor for every peak 0 .. 32768 (entry 0: 1.0, a silent segment is returned as it is)."""
    target = 32768 * 10 ** (-headroom_db / 20)
    out = np.ones(32769, dtype=np.float64)
    for p in range(1, 32769):
        boost = 20 * math.log(target / p, 10)
        out[p] = 10 ** (float(boost) / 20)
    return out


def post_gain(db=-3.0):
    return 10 ** (float(db) / 20)


def cut(audio, first, n):
    """audio[first : first + n] as Python's slicing clamps it."""
    return np.asarray(audio[first:first + n], dtype=np.int16)


def prepared_trial(audio, first, n, lead, normalize, table, post):
    """-> (int16 (n,), peak): `lead` zeros, then the first n - lead samples of the cut, normalised over the WHOLE cut."""
    c = cut(audio, first, n)
    pk = peak(c)
    if normalize:
        c = scale(scale(c, table[pk]), post)
    body = c[:n - lead]
    assert len(body) == n - lead, "the cut must hold the samples the shifted trial keeps"
    return np.concatenate([np.zeros(lead, dtype=np.int16), body]), pk


def prepared_list(audio, ranges, lead, normalize, table, post):
    """-> (concatenation, peaks int32, offsets)."""
    lead = np.broadcast_to(np.asarray(lead), (len(ranges),))
    outs, peaks = [], []
    for (first, n), ld, flag in zip(ranges, lead, normalize):
        x, pk = prepared_trial(audio, first, n, int(ld), bool(flag), table, post)
        outs.append(x)
        peaks.append(pk)
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in outs])]).astype(np.int64)
    return (np.concatenate(outs) if outs else np.zeros(0, np.int16)), np.array(peaks, dtype=np.int32), offsets


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).digest()
