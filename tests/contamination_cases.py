"""Cases of the contamination kernels (csrc/contamination.hip) for the tests (helper module, no tests in it).

How a call is cut -- frames into tiles of 32, tiles into chunks, lags into lag groups of the grid and lags per wave -- is decided
at run time from (W, C, L), and every loop of ``contam_corr_kernel`` depends on the cut.  ``NAMES`` lists the operators and
recordings that, together, reach chunks of several tiles with a shorter last chunk, one chunk for everything, every place the
mask can ride in (B = 1, 15, 16, 17, 31), the DC and the Nyquist bin, windows that are odd or no multiple of 4, frames that abut
or lie apart, one to three lag groups with idle waves, lags beyond the recording, full and one-frame last tiles, recordings with
no, one or a few kept frames, and the largest window the LDS holds.  Which cut a case really gets is NOT taken from here:
``spec(name).plan`` is what the case is there to reach, tests/test_cpu_contamination.py asks the library (``dss_contam_plan``)
and compares, tests/test_gpu_contamination.py asserts the same before it looks at a result, and both take operators, signals and
masks from this module so that they cannot drift apart.  Everything is seeded and generated, nothing is stored.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

import contamination_reference as ref

# op: keywords of ContaminationGPU and ref.Day; shape: (nperseg, hop, bin_lo, B, L, W);
# plan: (frames, tiles, chunks, tiles per chunk, lag groups Z, lags per wave)
Spec = collections.namedtuple("Spec", "name op T C shape plan")

SMALL = dict(fs=1000, window=0.016, spg_fs=250, band=(125, 312.5), max_lag=0.012)     # nperseg 16, hop 4, bins 2 .. 5, L 3


def _small(L):
    return {**SMALL, "max_lag": L / 250}


def _bins(lo, hi):
    """nperseg 64, hop 16, L 2; the band cut 1 Hz outside bins lo .. hi (15.625 Hz apart)."""
    return dict(fs=1000, window=0.064, spg_fs=62.5, band=(lo * 15.625 - 1, hi * 15.625 + 1), max_lag=0.032)


_APART = dict(fs=1000, window=0.018, spg_fs=40, band=(100, 400), max_lag=0.1)         # nperseg 18, hop 25, bins 2 .. 7, L 4
_ABUT = dict(fs=1000, window=0.018, spg_fs=1000 / 18, band=(100, 400), max_lag=0.072)  # hop 18

_TABLE = (
    # 32 tiles in 11 chunks of 3, the last of 2
    Spec("many_tiles", SMALL, 4068, 40, (16, 4, 2, 4, 3, 1014), (1014, 32, 11, 3, 1, 2)),
    # C Z >= 512: one workgroup per channel walks every tile
    Spec("one_chunk", SMALL, 292, 520, (16, 4, 2, 4, 3, 70), (70, 3, 1, 3, 1, 2)),
    # the default operator on a long recording: 61 tiles in 21 chunks of 3, the last of 1; two lag groups
    Spec("default_long", dict(fs=1000), 38680, 9, (200, 20, 14, 21, 25, 1925), (1925, 61, 21, 3, 2, 7)),
    # the planted case of contamination_reference: 2 tiles per chunk, the last chunk of 1
    Spec("planted", dict(fs=ref.PLANT_FS), ref.PLANT_T, ref.PLANT_C, (200, 20, 14, 21, 25, 991), (991, 31, 16, 2, 2, 7)),
    # the mask rides in place B of the audio operand; 5 lags on waves as 2, 2, 1, 0
    Spec("bins_1", _bins(32, 32), 768, 3, (64, 16, 32, 1, 2, 45), (45, 2, 2, 1, 1, 2)),         # the Nyquist bin alone
    Spec("bins_15", _bins(1, 15), 768, 3, (64, 16, 1, 15, 2, 45), (45, 2, 2, 1, 1, 2)),         # mask: last row of block 0
    Spec("bins_16", _bins(8, 23), 768, 3, (64, 16, 8, 16, 2, 45), (45, 2, 2, 1, 1, 2)),         # mask: first row of block 1
    Spec("bins_17", _bins(16, 32), 768, 3, (64, 16, 16, 17, 2, 45), (45, 2, 2, 1, 1, 2)),       # ends on the Nyquist bin
    Spec("bins_31", _bins(0, 30), 768, 3, (64, 16, 0, 31, 2, 45), (45, 2, 2, 1, 1, 2)),         # from DC; the pad is full
    # nperseg 37 (K4 = 40), hop 5, bins 3 .. 18 (18 is the last bin of an odd transform), 3 spare rows
    Spec("odd_window", dict(fs=1000, window=0.037, spg_fs=200, band=(80, 500), max_lag=0.02), 385, 3, (37, 5, 3, 16, 4, 70),
         (70, 3, 3, 1, 1, 3)),
    # hop 25 > K4 = 20: frames staged one by one; the rows between them are NaN.  5 spare rows
    Spec("apart", _APART, 998, 3, (18, 25, 2, 6, 4, 40), (40, 2, 2, 1, 1, 3)),
    Spec("abutting", _ABUT, 720, 3, (18, 18, 2, 6, 4, 40), (40, 2, 2, 1, 1, 3)),                # hop = nperseg < K4
    # nlag 1 / 33 / 65 / 81: Z 1 / 2 / 3 / 3, lags per wave 1 / 5 / 6 / 7
    Spec("lags_0", _small(0), 412, 2, (16, 4, 2, 4, 0, 100), (100, 4, 4, 1, 1, 1)),
    Spec("lags_16", _small(16), 412, 2, (16, 4, 2, 4, 16, 100), (100, 4, 4, 1, 2, 5)),
    Spec("lags_32", _small(32), 412, 2, (16, 4, 2, 4, 32, 100), (100, 4, 4, 1, 3, 6)),
    Spec("lags_40", _small(40), 412, 2, (16, 4, 2, 4, 40, 100), (100, 4, 4, 1, 3, 7)),
    Spec("largest_lag", _small(4096), 172, 1, (16, 4, 2, 4, 4096, 40), (40, 2, 2, 1, 257, 8)),
    # one frame; a full tile; a full tile and one frame; two full tiles (3 spare rows)
    Spec("frames_1", SMALL, 16, 2, (16, 4, 2, 4, 3, 1), (1, 1, 1, 1, 1, 2)),
    Spec("frames_32", SMALL, 140, 2, (16, 4, 2, 4, 3, 32), (32, 1, 1, 1, 1, 2)),
    Spec("frames_33", SMALL, 144, 2, (16, 4, 2, 4, 3, 33), (33, 2, 2, 1, 1, 2)),
    Spec("frames_64", SMALL, 271, 2, (16, 4, 2, 4, 3, 64), (64, 2, 2, 1, 1, 2)),
    Spec("keep_none", SMALL, 268, 2, (16, 4, 2, 4, 3, 64), (64, 2, 2, 1, 1, 2)),
    Spec("keep_one", SMALL, 268, 2, (16, 4, 2, 4, 3, 64), (64, 2, 2, 1, 1, 2)),
    Spec("keep_few", SMALL, 268, 2, (16, 4, 2, 4, 3, 64), (64, 2, 2, 1, 1, 2)),
)
NAMES = tuple(s.name for s in _TABLE) + ("lds_edge",)
# no lag of these has two pairs, so no correlation is defined and there is no r bound to take a median of
NO_CORRELATION = ("frames_1", "keep_none", "keep_one")
LDS_EDGE_FIRST_BIN = 10


def params_accepted(nperseg, hop, bin_lo, n_bins, max_lag):
    import ctypes as C
    from dss_amd import _lib, contamination
    p = contamination.ContamParams(nperseg, hop, bin_lo, n_bins, max_lag, 0)
    return _lib.load().dss_contam_check_params(C.addressof(p)) == 0


@functools.lru_cache(maxsize=None)
def lds_edge_nperseg():
    """The largest nperseg that dss_contam_check_params accepts at hop 1, 4 bins and L 0: bisection between a window that fits
    and the first one the header's limit of 2048 rules out anyhow (the LDS need grows with nperseg)."""
    lo, hi = 64, 2049
    assert params_accepted(lo, 1, LDS_EDGE_FIRST_BIN, 4, 0) and not params_accepted(hi, 1, LDS_EDGE_FIRST_BIN, 4, 0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if params_accepted(mid, 1, LDS_EDGE_FIRST_BIN, 4, 0):
            lo = mid
        else:
            hi = mid
    return lo


def spec(name) -> Spec:
    if name == "lds_edge":                           # 33 frames of one channel; the band cut half a bin outside bins 10 .. 13
        n = lds_edge_nperseg()
        op = dict(fs=1000, window=n / 1000, spg_fs=1000, band=(9.5 * 1000 / n, 13.5 * 1000 / n), max_lag=0.0)
        return Spec(name, op, n + 32, 1, (n, 1, LDS_EDGE_FIRST_BIN, 4, 0, 33), (33, 2, 2, 1, 1, 1))
    return _TABLE[NAMES.index(name)]


def _keep(name, T):
    """The per-sample mask of a case, or None."""
    keep = np.ones(T, dtype=bool)
    if name == "many_tiles":                         # frames of 16 rows every 4: frame t is rows 4 t .. 4 t + 15
        keep[390] = False                            # frames 94 .. 97: across the edge of tiles 2 and 3, which is a chunk edge
        keep[640:780] = False                        # every row of frames 160 .. 191, tile 5 (and frames 157 .. 159, 192 .. 194)
        keep[T - 1] = False                          # only the last frame
    elif name == "default_long":                     # frames of 200 rows every 20
        keep[1920] = False                           # frames 87 .. 96: across the edge of tiles 2 and 3, a chunk edge
        keep[T - 1] = False
    elif name == "planted":
        from dss_amd.contamination import detect_artifacts
        return ~detect_artifacts(ref.planted_case(True)[0], ref.PLANT_FS)
    elif name.startswith("lags_"):
        keep[200] = False                            # frames 47 .. 50
    elif name == "keep_none":
        keep[::16] = False                           # one row of every frame
    elif name == "keep_one":
        keep[:] = False
        keep[160:176] = True                         # frame 40
    elif name == "keep_few":
        keep[:] = False
        keep[80:108] = True                          # frames 20 .. 23
    else:
        return None
    return keep


@functools.lru_cache(maxsize=None)
def build(name):
    """(op, brain (T, C), audio (T,), keep or None), read-only.  Seeded noise channels of scale 0.5 to 20 with offsets, 0.05 x
    the audio leaking into one channel, and an audio with an offset, so that the DC bin is large and the centring matters.
    one_chunk's channels are columns 2 .. 521 of rows of 523; apart's rows that no frame covers are NaN on both sides; lds_edge's
    first and last 32 rows are louder."""
    s = spec(name)
    if name == "planted":
        brain, audio = ref.planted_case(True)
    else:
        rng = np.random.default_rng(7300 + NAMES.index(name))
        wide = s.C + 3 if name == "one_chunk" else s.C
        brain = rng.standard_normal((s.T, wide)) * rng.uniform(0.5, 20.0, size=wide) + rng.uniform(-3, 3, size=wide)
        audio = 50.0 * rng.standard_normal(s.T) + 30.0
        brain[:, wide // 2] += 0.05 * audio
        if name == "apart":
            nperseg, hop, W = s.shape[0], s.shape[1], s.shape[5]
            covered = np.zeros(s.T, dtype=bool)
            for t in range(W):
                covered[t * hop:t * hop + nperseg] = True
            assert 0 < covered.sum() == W * nperseg < s.T
            brain[~covered] = np.nan
            audio[~covered] = np.nan
        if name == "lds_edge":                       # at hop 1 the frames share all rows but one, whose window weight is 0.08: the
            edge = np.r_[0:32, s.T - 32:s.T]         # rows that leave and enter are 200 x louder, so that the magnitudes vary
            brain[edge] *= 200.0                     # from frame to frame by about their own size and the variances do not cancel
            audio[edge] *= 200.0
        if name == "one_chunk":
            brain = brain[:, 2:2 + s.C]
    keep = _keep(name, s.T)
    for v in (brain, audio, keep):
        if v is not None:
            v.setflags(write=False)
    assert brain.shape == (s.T, s.C) and audio.shape == (s.T,)
    return s.op, brain, audio, keep


@functools.lru_cache(maxsize=None)
def day(name):
    """The reference's spectrograms of a case, computed once and shared."""
    op, brain, audio, keep = build(name)
    return ref.Day(brain, audio, keep=keep, **op)


def shape_of(d):
    return (d.nperseg, d.hop, int(d.bins[0]), len(d.bins), d.L, d.W)


def kept_mean(d):
    """The mean of the kept audio frames, the shift the library subtracts; zeros when no frame is kept."""
    return d.A[d.fm].mean(axis=0) if d.fm.any() else np.zeros(len(d.bins))


def check_exact(name, n, shift, sums, r):
    """What holds without any tolerance, for the reference's sums and for the library's alike.  n (lags,), shift (B,), sums a
    dict of sa, saa, sb, sbb, sab, r (lags, C, B, B)."""
    L = (len(n) - 1) // 2
    W = spec(name).shape[5]
    assert np.all(n == np.floor(n)) and np.all(n >= 0) and np.all(n <= W)
    lags = np.arange(-L, L + 1)
    empty = n == 0
    assert np.all(empty[np.abs(lags) >= W])                                          # no pair that far apart
    for key in ("sa", "saa", "sb", "sbb", "sab"):
        assert not sums[key][empty].any(), key                                        # exact zeros, no NaN
    assert np.all(np.isnan(r[n < 2]))
    if name == "keep_none":
        assert not n.any() and not shift.any()
    if name == "keep_one" or name == "frames_1":
        assert n[L] == 1 and n.sum() == 1
    if name in NO_CORRELATION:
        assert np.all(np.isnan(r))
    else:
        assert not np.all(np.isnan(r))
    if name == "keep_few":
        assert list(n) == [1, 2, 3, 4, 3, 2, 1]
    if name == "largest_lag":
        assert list(n[L - 39:L + 40]) == [40 - abs(l) for l in range(-39, 40)] and n.sum() == 40 * 40
