"""Cases of the HGA kernels (csrc/hga_kernels.hip) for the tests (helper module, no tests in it).

The golden vectors sit on the reference's one configuration: 8 sections per cascade, 50 ms / 10 ms windows at 1 kHz, 64 or 128
channels.  The kernels accept more, and take other branches when they get it: with fewer than 8 sections some lanes of a DPP row
hold no section and the last section is not lane 15; with C no multiple of 16 and several streams a block's 16 columns belong to
two or three streams; the one-launch forms exist only while their LDS ring fits, and windows past the 128-entry table take
their rows from the float32 arithmetic directly; the front end, the patch, the statistics and the wire kernels have unrolled
loops with remainders and tiles with a largest size.  The tables below name the smallest shapes that reach each of these, and
the references the results are held to -- the oracle (oracle/hga_oracle.c, pinned to the reference's own module by
tests/test_oracle_hga.py), scipy and numpy; everything is seeded and computed at test time, nothing is stored.

Which form serves a case is NOT taken from here: ``Case.plan`` is what the case is there to reach, tests/test_cpu_hga_cases.py
asks the library (``dss_hga_plan``, the helper the launch code itself uses) and compares, and tests/test_gpu_hga_cases.py runs
the same cases.  The bounds (the ring, the front end's tile, the wire tile) are restated from the code's formulas in
``ring_rows``, ``FRONT_MAX_C_RAW`` and ``wire_fits`` and asserted against the library where it can tell without a device.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

from dss_amd.synthetic import synthetic_ecog

# plan: (frame_length, shift, overlap, ring_rows, ring_bytes, fused); frames: the oracle's frames per packet
Case = collections.namedtuple("Case", "name group S C fs wl ws order packets plan frames")

RING_LIMIT = 40 * 1024          # bytes of LDS the one-launch kernels leave for their ring (dss_hga_ring, csrc/dss_common.h)
WTAB = 128                      # HGF_WTAB: windows whose rows the one-launch kernels tabulate


def ring_rows(frame_length, shift):
    """A frame, one shift, one tile of 64 steps and 2 rows, rounded up to a multiple of 8."""
    return (frame_length + shift + 66 + 7) & ~7


def _plan(frame_length, shift):
    rows = ring_rows(frame_length, shift)
    return (frame_length, shift, frame_length - shift, rows, rows * 128, int(rows * 128 <= RING_LIMIT))


DEFAULT = (1000, 0.05, 0.01)
_ORDER_PACKETS = (3, 100, 1000, 397)            # 3 < 2 nsec - 1 for every order but 1, and shorter than a frame
_TAIL_PACKETS = (30, 100, 17, 64, 250)          # 30 and 17 are shorter than the overlap of 40 rows
_RING_PACKETS = (3, 97, 1000, 400)              # 1500 rows through a ring of 320: it wraps more than three times
_D = _plan(50, 10)

_TABLE = tuple(
    # sections per cascade: lanes 2 k .. 15 of a row hold no section, the last section is lane 2 k - 1
    [Case(f"order_{k}", "orders", 2, 5, *DEFAULT, k, _ORDER_PACKETS, _D, (1, 10, 100, 39)) for k in (1, 2, 3, 5, 7, 8)] + [
    # blocks of 16 (stream, channel) columns that span streams
    Case("tail_3x5", "tails", 3, 5, *DEFAULT, 8, _TAIL_PACKETS, _D, (1, 10, 1, 6, 25)),       # one block, three streams
    Case("tail_7x5", "tails", 7, 5, *DEFAULT, 8, _TAIL_PACKETS, _D, (1, 10, 1, 6, 25)),       # 35 columns: the last block has 3
    Case("tail_2x24", "tails", 2, 24, *DEFAULT, 8, _TAIL_PACKETS, _D, (1, 10, 1, 6, 25)),     # the stream edge inside block 1
    Case("tail_3x40", "tails", 3, 40, *DEFAULT, 8, _TAIL_PACKETS, _D, (1, 10, 1, 6, 25)),     # window kernel: 32 + 8 channels
    # fs 512, 0.375 s windows (192 rows; both exact in float32): the last shift whose ring fits, and the first that does not
    Case("ring_last_fused_8", "ring", 2, 5, 512, 0.375, 62 / 512, 8, _RING_PACKETS, _plan(192, 62), (1, 1, 16, 6)),
    Case("ring_last_fused_3", "ring", 2, 5, 512, 0.375, 62 / 512, 3, _RING_PACKETS, _plan(192, 62), (1, 1, 16, 6)),
    Case("ring_first_fallback_8", "ring", 2, 5, 512, 0.375, 63 / 512, 8, _RING_PACKETS, _plan(192, 63), (1, 1, 15, 6)),
    Case("ring_first_fallback_3", "ring", 2, 5, 512, 0.375, 63 / 512, 3, _RING_PACKETS, _plan(192, 63), (1, 1, 15, 6)),
    # 200 windows in one call: entries 128 .. 199 are past the table
    Case("beyond_table", "table", 2, 5, 1000, 0.025, 0.005, 8, (100, 1000), _plan(25, 5), (16, 200)),
])
NAMES = tuple(c.name for c in _TABLE)
GROUPS = ("orders", "tails", "ring", "table")


def case(name) -> Case:
    return _TABLE[NAMES.index(name)]


def names(group):
    return tuple(c.name for c in _TABLE if c.group == group)


@functools.lru_cache(maxsize=None)
def filters(fs, order):
    """The two cascades of ``order`` sections each and their unit-step states, as HgaExtractorGPU and the oracle take them."""
    from dss_amd.hga import design_filters
    hg, fh, zi_hg, zi_fh = design_filters(fs, order=order)
    assert hg.shape == fh.shape == (order, 6)
    for a in (hg, fh, zi_hg, zi_fh):
        a.setflags(write=False)
    return {"sos_hg": hg, "sos_fh": fh, "zi_hg": zi_hg, "zi_fh": zi_fh}


def filter_tuple(fs, order):
    f = filters(fs, order)
    return f["sos_hg"], f["sos_fh"], f["zi_hg"], f["zi_fh"]


@functools.lru_cache(maxsize=None)
def signal(name):
    """(S, T, C) float64, read-only: every stream its own seeded recording."""
    c = case(name)
    x = np.stack([synthetic_ecog(8100 + 50 * NAMES.index(name) + s, sum(c.packets), c.C, fs=c.fs) for s in range(c.S)])
    x.setflags(write=False)
    return x


def zscore(C):
    """Distinct per-channel means and spreads."""
    rng = np.random.default_rng(8300 + C)
    return rng.standard_normal(C) * 3.0, rng.uniform(0.5, 2.0, C)


class Chain:
    """oracle_hga_extract's steps one after the other (the two cascades, the frame buffer, the windowed power), so that the mean
    power is at hand as well as its log; tests/test_cpu_hga_cases.py holds the log to ``oracle.extractor`` itself."""

    def __init__(self, oracle, filt, C, fs, wl, ws):
        self.o, self.f, self.fs, self.wl, self.ws = oracle, filt, fs, wl, ws
        self.zi = [np.ascontiguousarray(np.repeat(filt[k][:, :, None], C, axis=2)) for k in ("zi_hg", "zi_fh")]
        self.fb = oracle.framebuffer(wl, ws, fs, C)

    def extract(self, x):
        """(n, C) -> (mean power + 0.01, its log), (W, C) each."""
        y, self.zi[0] = self.o.sosfilt(self.f["sos_hg"], x, self.zi[0])
        y, self.zi[1] = self.o.sosfilt(self.f["sos_fh"], y, self.zi[1])
        rows = self.fb.insert(y)
        return (self.o.log_power(rows, self.fs, self.wl, self.ws, mean_only=True), self.o.log_power(rows, self.fs, self.wl, self.ws))


_REFERENCE = {}


def reference(oracle, name):
    """The oracle's frames of a case, computed once and shared: {"power", "log": one (S, W, C) array per packet, "whole_power",
    "whole_log": (S, W, C) of the recording as ONE chunk into a fresh extractor, which is what a trial is}."""
    if name not in _REFERENCE:
        c, x = case(name), signal(name)
        f = filters(c.fs, c.order)
        per_stream, whole = [], []
        for s in range(c.S):
            ch, pos, parts = Chain(oracle, f, c.C, c.fs, c.wl, c.ws), 0, []
            for n in c.packets:
                parts.append(ch.extract(x[s, pos:pos + n]))
                pos += n
            per_stream.append(parts)
            whole.append(Chain(oracle, f, c.C, c.fs, c.wl, c.ws).extract(x[s]))
        ref = {"power": [np.stack([per_stream[s][k][0] for s in range(c.S)]) for k in range(len(c.packets))],
               "log": [np.stack([per_stream[s][k][1] for s in range(c.S)]) for k in range(len(c.packets))],
               "whole_power": np.stack([w[0] for w in whole]), "whole_log": np.stack([w[1] for w in whole])}
        for v in ref.values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
        _REFERENCE[name] = ref
    return _REFERENCE[name]


# ---- front ends (hga_frontend_kernel) ------------------------------------------------------------------------------------
# The kernel's dynamic LDS: 32 rows of c_raw doubles, 32 x 4 means, 4 c_raw member columns (ints) = 272 c_raw + 1024 bytes <= 64 KB
FRONT_MAX_C_RAW = (64 * 1024 - 1024) // 272
FRONT_ROWS = (1, 31, 32, 33, 100)               # packets of one stream: S n rows, around the kernel's tile of 32
Front = collections.namedtuple("Front", "name c_raw C src_col grid_of comp_lists")


def _front(seed, name, c_raw, C, sizes, unreferenced=(), repeat=False):
    """Seeded layout: grid g averages sizes[g] raw columns in a shuffled order; the channels take the grids in turn."""
    rng = np.random.default_rng(8500 + seed)
    src = rng.permutation(c_raw)[:C]
    if repeat:
        src[C - 1] = src[0]
    grid_of = np.arange(C) % len(sizes)
    grid_of[list(unreferenced)] = -1
    comp = [rng.permutation(c_raw)[:k] for k in sizes]
    return Front(name, c_raw, C, src.astype(np.int64), grid_of.astype(np.int64), comp)


FRONTS = (
    _front(0, "front_one_grid", 20, 6, (8,)),
    _front(1, "front_three_grids", 40, 9, (1, 7, 9)),
    _front(2, "front_four_grids", 50, 12, (8, 17, 1, 7)),
    _front(3, "front_unreferenced", 30, 9, (9, 16), unreferenced=(1, 4, 7)),          # a third of the channels pass through
    _front(4, "front_repeated_source", 12, 8, (7, 8), repeat=True),
    _front(5, "front_largest", FRONT_MAX_C_RAW, 64, (118, 119)),
)
FRONT_NAMES = tuple(f.name for f in FRONTS)


def front(name) -> Front:
    return FRONTS[FRONT_NAMES.index(name)]


def frontend_reference(raw, src_col, grid_of, comp_lists):
    """(..., c_raw) -> (..., C): per grid a sequential float64 sum of the member columns in list order, one division, and per
    channel one subtraction (none for grid -1)."""
    raw = np.asarray(raw, dtype=np.float64)
    means = []
    for cols in comp_lists:
        acc = np.zeros(raw.shape[:-1])
        for col in cols:
            acc = acc + raw[..., col]
        means.append(acc / len(cols))
    out = np.empty(raw.shape[:-1] + (len(src_col),))
    for c, (col, g) in enumerate(zip(src_col, grid_of)):
        out[..., c] = raw[..., col] - means[g] if g >= 0 else raw[..., col]
    return out


def front_raw(name, S=1):
    f = front(name)
    rng = np.random.default_rng(8600 + FRONT_NAMES.index(name))
    return rng.standard_normal((S, sum(FRONT_ROWS), f.c_raw)) * 40.0 + rng.uniform(-5, 5, f.c_raw)


# ---- patches (hga_patch_kernel) -------------------------------------------------------------------------------------------
PATCH_C = 160
PATCH_NEIGHBOURS = (1, 7, 8, 9, 15, 16, 17, 24, 127)
PATCH_TRIALS = ((0, 30), (40, 55), (100, 65), (150, 133))          # (start, rows): 1 (zero-padded), 1, 2 and 9 frames
PATCH_FRAMES = (1, 1, 2, 9)
PATCH_T = 300


def patches(C=PATCH_C, counts=PATCH_NEIGHBOURS):
    """[(column, neighbours)]: columns 0, 1, ... are patched, each from its own shuffled draw of the others."""
    rng = np.random.default_rng(8700)
    free = np.arange(len(counts), C)
    return [(k, rng.permutation(free)[:n]) for k, n in enumerate(counts)]


def numpy_patch(frames, bounds, patch_list):
    """BadChannelCorrection trial by trial, as numpy evaluates it on each trial's frames."""
    want = frames.copy()
    for a, b in zip(bounds, bounds[1:]):
        for dst, nb in patch_list:
            want[a:b, dst] = np.mean(frames[a:b][:, nb], axis=1)
    return want


# ---- statistics (hga_colstats_kernel) -------------------------------------------------------------------------------------
STATS_N = (1, 2, 8, 9, 10, 17)
STATS_C = (1, 63, 64, 65, 130)
STATS_ONE_COLUMN_N = (128, 129, 300, 1000)      # C = 1 only: numpy halves a contiguous run of more than 128 elements


def stats_frames(N, C):
    """Seeded (N, C) frames; the last column has mean 1e6 and spread 1e-3."""
    x = np.random.default_rng(8800 + 131 * N + C).standard_normal((N, C)) * 3.0 + 5.0
    x[:, C - 1] = 1e6 + 1e-3 * x[:, C - 1]
    return np.ascontiguousarray(x)


# ---- wire packets (hga_wire_kernel) ---------------------------------------------------------------------------------------
WIRE_LIMIT = 64 * 1024                       # bytes of the kernel's float32 tile: one stream's packet
WIRE = ((64, 1, True), (129, 127, True), (129, 128, False), (64, 256, True), (64, 257, False))      # (C, n, accepted)


def wire_fits(C, n):
    return C * n * 4 <= WIRE_LIMIT
