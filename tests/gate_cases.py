"""Cases of the speech-gate kernels (csrc/speech_gate.hip, csrc/dss_gate.cpp) for the tests (helper module, no tests in it).

tests/golden/gate.npz and the tests on it sit in one corner: threshold 0.6, a smoothing window of at most 11 labels, at most 70
features, random label runs.  ``CASES`` names the smallest runs that reach the rest of what the kernels do:

  window     the label window as a 64-bit mask carried in two ints: the first window with a bit in the high word (33) and the
             largest one taken (63); ``REFUSED_SMOOTHING_CONTEXT`` is the first one refused
  threshold  popcount / window >= threshold in float64: on the tie (3 of 5 at 0.6, 1 of 3 at 1/3, 2 of 3 at 2/3, 49 of 49 at 1.0,
             where a multiply by the reciprocal 1/49 falls short of 1.0), and at both ends (0.0: nothing ever closes; 1.5: never speech)
  width      the copy-out's (row, column) walk with carry, 256 elements a step and four steps in flight: C = 1 and 256 (no column
             step), above 256 (no row step), the neighbours of 64 and 256, totals that end inside the unroll
  empty      a segment of 0 rows: 2 * context + speech run = 0 modulo the ring
  capacity   exactly ``max_events`` segments closed by one push
  values     float64 -> float32 at the ring's entry: overflow, the subnormal range, ties to even, -0.0, inf, NaN
  pushes     the same frames one at a time and in one push; a segment of more than 16 x 256 elements; 130 streams with rings
             of their own

Every case is held to tests/golden/gate_cases.npz, which the reference's own VoiceActivityDetectionSmoothing + SpeechSegmentHistory
computed (tools/make_golden_gate_cases.py).  ``reach`` is what a case is there to reach, as ``observe`` counts it from a run of
oracle/speech_gate_oracle.py: tests/test_cpu_gate_cases.py computes it again and compares, so that no case passes on the
device without reaching its branch.

Frames and labels are never stored twice: labels are in the fixture AND come from ``labels`` here (the CPU test compares them),
frames come from ``frames`` alone.  Each stream of a case has its own seed.
"""
from __future__ import annotations

import collections
import functools
import zlib

import numpy as np

THREADS = 256                    # GATE_THREADS: elements one step of the copy-out moves
UNROLL = 4                       # steps in flight per thread
COLLECT_MAX = 64                 # DSS_GATE_COLLECT_MAX: segments per launch of gate_collect_kernel
COLLECT_ROWS = 16                # gridDim.y of gate_collect_kernel: 16 x 256 elements per trip
REFUSED_SMOOTHING_CONTEXT = 32   # window 65: the first one the 64-bit mask cannot hold

Case = collections.namedtuple("Case", "name C N context smoothing_context threshold max_frames S pushes reach note")


def max_events(max_frames, context):
    """dss_gate_create's capacity restated: a segment closes on the context-th non-speech frame after at least one speech
    frame.  The first one of a push may close on its first frame (a carried run); each later one needs a speech frame and
    ``context`` non-speech frames, or a speech frame and one non-speech frame without context."""
    return max_frames // (context + 1) + 1 if context > 0 else (max_frames + 1) // 2


CASES = (
    # ---- the label window
    Case("mask_33", 3, 64, 2, 16, 0.6, 7, 3, 300, (("segments", 20), ("bit_32", True)),
         "window 33: the first with a bit in the mask's high word"),
    Case("mask_63", 3, 64, 2, 31, 0.6, 7, 3, 400, (("segments", 23), ("bit_62", True)),
         "window 63: the largest one taken"),
    # ---- the threshold
    Case("thr_one_49", 3, 200, 2, 24, 1.0, 7, 3, 400, (("segments", 16), ("count_49_of_49", True), ("count_48_of_49", True)),
         "49 / 49 >= 1.0 holds, 49 * (1 / 49) >= 1.0 does not"),
    Case("thr_zero", 3, 64, 2, 2, 0.0, 7, 2, 60, (("segments", 0), ("all_speech", True)), "every frame is speech, nothing ever closes"),
    Case("thr_above_one", 3, 64, 2, 2, 1.5, 7, 2, 60, (("segments", 0), ("no_speech", True)), "never speech"),
    Case("tie_3of5", 3, 64, 2, 2, 0.6, 7, 2, 200, (("segments", 98), ("on_tie", 305)), "3 / 5 >= 0.6"),
    Case("tie_1of3", 3, 64, 2, 1, 1.0 / 3.0, 7, 2, 200, (("segments", 96), ("on_tie", 384)), "1 / 3 >= 1 / 3"),
    Case("tie_2of3", 3, 64, 2, 1, 2.0 / 3.0, 7, 2, 200, (("segments", 124), ("on_tie", 389)), "2 / 3 >= 2 / 3"),
    # ---- the copy-out walk: dr = 256 / C, dc = 256 - dr * C
    Case("width_1", 1, 41, 2, 0, 0.6, 7, 2, 120, (("segments", 37), ("not_multiple_of_256", True), ("above_1024", False)), "dr 256, dc 0"),
    Case("width_63", 63, 41, 2, 0, 0.6, 7, 2, 120, (("segments", 39), ("not_multiple_of_256", True), ("above_1024", True)), "dr 4, dc 4"),
    Case("width_64", 64, 41, 2, 0, 0.6, 7, 2, 120, (("segments", 37), ("not_multiple_of_256", True), ("above_1024", True)), "dr 4, dc 0"),
    Case("width_65", 65, 41, 2, 0, 0.6, 7, 2, 120, (("segments", 43), ("not_multiple_of_256", True), ("above_1024", True)), "dr 3, dc 61"),
    Case("width_255", 255, 41, 2, 0, 0.6, 7, 2, 120, (("segments", 30), ("not_multiple_of_256", True), ("above_1024", True)), "dr 1, dc 1"),
    Case("width_256", 256, 41, 2, 0, 0.6, 7, 2, 120, (("segments", 37), ("not_multiple_of_256", False), ("above_1024", True)), "dr 1, dc 0"),
    Case("width_257", 257, 41, 2, 0, 0.6, 7, 2, 120, (("segments", 33), ("not_multiple_of_256", True), ("above_1024", True)), "dr 0, dc 256"),
    Case("width_300", 300, 41, 2, 0, 0.6, 7, 2, 120, (("segments", 40), ("not_multiple_of_256", True), ("above_1024", True)), "dr 0, dc 256"),
    # ---- segments of 0 rows
    Case("zero_ctx1", 5, 8, 1, 0, 0.6, 5, 2, 8, (("segments", 6), ("empty_segments", 2)), "2 * 1 + 6 = 8: a run of 6 among runs of 7 and 5"),
    Case("zero_ctx0", 5, 8, 0, 0, 0.6, 5, 2, 12, (("segments", 8), ("empty_segments", 4)), "runs of 8 and 16 among runs of 9 and 7"),
    # ---- exactly max_events segments in one push
    Case("cap_ctx0_w7", 4, 16, 0, 0, 0.6, 7, 2, 3, (("segments", 10), ("most_in_a_push", 4)), "(7 + 1) / 2 = 4"),
    Case("cap_ctx0_w8", 4, 16, 0, 0, 0.6, 8, 2, 3, (("segments", 10), ("most_in_a_push", 4)), "(8 + 1) / 2 = 4"),
    Case("cap_ctx2_w8", 4, 16, 2, 0, 0.6, 8, 2, 3, (("segments", 8), ("most_in_a_push", 3)), "8 / 3 + 1 = 3"),
    # ---- float64 -> float32
    Case("values", 14, 23, 3, 1, 0.6, 7, 2, 80, (("segments", 30), ("special_values_emitted", 14)), "every special value in an emitted row"),
    # ---- push sizes and stream counts
    Case("one_by_one", 5, 32, 2, 1, 0.6, 1, 2, 50, (("segments", 8),), "50 frames, one per push"),
    Case("whole_50", 5, 32, 2, 1, 0.6, 50, 2, 1, (("segments", 8), ("most_in_a_push", 4)), "the same 50 frames in one push"),
    Case("long_64", 64, 128, 2, 0, 0.6, 8, 2, 14, (("segments", 2), ("above_4096", True)),
         "a run of 100 frames: 104 x 64 elements, a second trip of gate_collect_kernel's stride loop"),
    Case("streams_130", 5, 32, 2, 1, 0.6, 6, 130, 13, (("segments", 245), ("streams_closing_on_last_run", 130)),
         "130 streams: the first count beyond the pipeline's 128; every stream closes a segment on the same push"),
)
NAMES = tuple(c.name for c in CASES)
WIDTH_NAMES = tuple(n for n in NAMES if n.startswith("width_"))
TIE_COUNT = {"tie_3of5": 3, "tie_1of3": 1, "tie_2of3": 2}      # the window count that sits exactly on the case's threshold


def case(name) -> Case:
    return CASES[NAMES.index(name)]


# ---- labels ---------------------------------------------------------------------------------------------------------------
# random runs: per stream s the flip probability FLIP[name][s % len]; written scripts: one string per push
FLIP = {"mask_33": (0.015, 0.02, 0.03), "mask_63": (0.015, 0.02, 0.03), "thr_one_49": (0.008, 0.01, 0.012),
        "thr_zero": (0.1,), "thr_above_one": (0.1,), "tie_3of5": (0.25, 0.3), "tie_1of3": (0.25, 0.3), "tie_2of3": (0.25, 0.3),
        "values": (0.1, 0.15)}
FLIP.update({n: (0.08,) for n in WIDTH_NAMES})

SCRIPT = {
    "zero_ctx1": ("00111", "11110", "00111", "11100", "01111", "10000", "00000", "00000"),          # runs of 7, 6 (0 rows), 5
    "zero_ctx0": ("01111", "11111", "00111", "11111", "00111", "11111", "11111", "11100",           # runs of 9, 8 (0 rows), 16 (0 rows), 7
                  "01111", "11100", "00000", "00000"),
    "cap_ctx0_w7": ("0001111", "0101010", "0011000"),
    "cap_ctx0_w8": ("00001111", "01010101", "00000000"),
    "cap_ctx2_w8": ("00011110", "01001001", "00000000"),
    "long_64": ("00011111",) + ("11111111",) * 11 + ("11111110", "00000000"),
    "one_by_one": tuple("00011111100010011111111110000110100000001111000000"),
    "whole_50": ("00011111100010011111111110000110100000001111000000",),
}
SAME_DATA = {"whole_50": "one_by_one"}        # the case whose seeds a case borrows: the same frames, pushed differently
STREAMS_130_FRAMES, STREAMS_130_LAST_RUN_END = 48, 40


def seed(name, stream):
    """One seed per (case, stream), from the case's name (a new row in the table moves no other case's data); stream -1 seeds
    what the streams of a case share (the push sizes)."""
    return 1000 * (zlib.crc32(SAME_DATA.get(name, name).encode()) % 9973) + 1 + stream


@functools.lru_cache(maxsize=None)
def sizes(name):
    """Frames of every push, shared by a case's streams (they advance in lock-step).  Read-only."""
    c = case(name)
    if name in SCRIPT:
        out = np.array([len(p) for p in SCRIPT[name]], dtype=np.int32)
    elif name == "streams_130":
        rng = np.random.default_rng(seed(name, -1))
        out = []
        while sum(out) < STREAMS_130_FRAMES:
            out.append(min(int(rng.integers(1, c.max_frames + 1)), STREAMS_130_FRAMES - sum(out)))
        out = np.array(out, dtype=np.int32)
    else:
        out = np.random.default_rng(seed(name, -1)).integers(1, c.max_frames + 1, c.pushes).astype(np.int32)
    assert len(out) == c.pushes and out.min() >= 1 and out.max() <= c.max_frames, (name, len(out))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def labels(name, stream):
    """Raw labels (frames,) int8 of one stream.  Read-only."""
    T = int(sizes(name).sum())
    if name in SCRIPT:
        out = np.array([int(ch) for p in SCRIPT[name] for ch in p], dtype=np.int8)
    elif name == "streams_130":
        # a first run of the stream's own, then a run of the stream's own start that ends on the same frame in every stream
        rng = np.random.default_rng(seed(name, stream))
        out = np.zeros(T, dtype=np.int8)
        a = int(rng.integers(2, 8))
        out[a:a + int(rng.integers(1, 12))] = 1
        out[int(rng.integers(24, 34)):STREAMS_130_LAST_RUN_END] = 1
    else:
        rng = np.random.default_rng(seed(name, stream))
        p = FLIP[name][stream % len(FLIP[name])]
        flips = rng.random(T) < p
        out = ((int(rng.integers(0, 2)) + np.cumsum(flips)) % 2).astype(np.int8)
    out.setflags(write=False)
    return out


# ---- frames ---------------------------------------------------------------------------------------------------------------
F32_MAX = float(np.finfo(np.float32).max)
HALF_SUBNORMAL = 2.0 ** -150                   # half the smallest float32 subnormal: a tie between 0 and 2^-149, to even = 0
# (float64 value, the float32 bits it must become)
SPECIAL = (
    (3.5e38, 0x7f800000), (-3.5e38, 0xff800000),                       # beyond float32: +-inf
    (F32_MAX, 0x7f7fffff),                                             # float32's maximum, exactly
    (1e-40, 0x000116c2), (-1e-40, 0x800116c2),                         # the subnormal range
    (1e-46, 0x00000000),                                               # under half the smallest subnormal
    (HALF_SUBNORMAL, 0x00000000), (float(np.nextafter(HALF_SUBNORMAL, 1.0)), 0x00000001),
    (1.0 + 2.0 ** -24, 0x3f800000), (1.0 + 3.0 * 2.0 ** -24, 0x3f800002),      # ties, rounded to even
    (-0.0, 0x80000000),
    (float("inf"), 0x7f800000), (float("-inf"), 0xff800000),
    (float(np.nan), 0x7fc00000),                                       # the canonical quiet NaN only
)


@functools.lru_cache(maxsize=None)
def frames(name, stream):
    """Frames (frames, C) float64 of one stream: N(0, 9) values that are NOT float32 values, so the cast rounds; in ``values``
    about half the entries are replaced by the special values.  Read-only."""
    c = case(name)
    T = int(sizes(name).sum())
    rng = np.random.default_rng(seed(name, stream) + 500)
    out = rng.standard_normal((T, c.C)) * 3.0
    if name == "values":
        which = rng.integers(0, len(SPECIAL), (T, c.C))
        put = rng.random((T, c.C)) < 0.5
        out[put] = np.array([v for v, _ in SPECIAL])[which[put]]
    out.setflags(write=False)
    return out


def to_float32(x):
    """numpy's own float64 -> float32 cast, without its warnings about the overflows and NaNs that ``values`` is there for."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(x).astype(np.float32)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def push_bounds(name):
    """[(first frame, end frame)] of every push."""
    e = np.cumsum(sizes(name))
    return list(zip((e - sizes(name)).tolist(), e.tolist()))


# ---- the fixture -------------------------------------------------------------------------------------------------------------
class Expected:
    """One case of tests/golden/gate_cases.npz: for stream s and push k the speech count and the segments, each as the indices
    of the input frames its rows copy (-1: a row of the initially zeroed rings)."""

    def __init__(self, g, name):
        c = case(name)
        self.case = c
        self.sizes = g[f"{name}_sizes"]
        self.labels = g[f"{name}_labels"]                      # (S, frames) int8
        self.speech = g[f"{name}_speech"]                      # (S, pushes) int32
        seg_stream, seg_push, seg_len = g[f"{name}_seg_stream"], g[f"{name}_seg_push"], g[f"{name}_seg_len"]
        rows = g[f"{name}_rows"]
        assert rows.shape == (int(seg_len.sum()),) and self.labels.shape == (c.S, int(self.sizes.sum()))
        self.segments = {}                                     # (stream, push) -> [row indices of each segment]
        at = 0
        for s, k, n in zip(seg_stream.tolist(), seg_push.tolist(), seg_len.tolist()):
            self.segments.setdefault((s, k), []).append(rows[at:at + n])
            at += n
        self.n_segments = len(seg_len)

    def rows_of(self, stream, push):
        return self.segments.get((stream, push), [])

    def segment(self, name, stream, index):
        """The float32 rows a segment with these row indices holds."""
        return rows_from(frames32(name, stream), index)


@functools.lru_cache(maxsize=None)
def frames32(name, stream):
    out = to_float32(frames(name, stream))
    out.setflags(write=False)
    return out


def rows_from(frames_any, index):
    """frames.astype(float32)[index], zeros where the index is -1."""
    f32 = to_float32(frames_any)
    out = np.zeros((len(index), f32.shape[1]), dtype=np.float32)
    keep = np.asarray(index) >= 0
    out[keep] = f32[np.asarray(index)[keep]]
    return out


# ---- what a case reaches --------------------------------------------------------------------------------------------------------
def observe(name, make_oracle):
    """Run every stream of a case through ``make_oracle(C, N, context, smoothing_context, threshold)`` frame by frame and count
    what the case is there for.  -> (dict of everything ``reach`` may name, segments per stream and push as lists of arrays)."""
    c = case(name)
    W = 2 * c.smoothing_context + 1
    o = dict(segments=0, empty_segments=0, most_in_a_push=0, on_tie=0, streams_closing_on_last_run=0)
    seen_counts, hi_bits, n_speech_all, frames_all, elements = set(), set(), 0, 0, []
    emitted, last, per_stream = set(), [], []
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):      # the casts ``values`` is there for
        for s in range(c.S):
            g = make_oracle(c.C, c.N, c.context, c.smoothing_context, c.threshold)
            f, lab = frames(name, s), labels(name, s)
            out = []
            last_push_segments = -1                                 # the last push on which this stream closed a segment
            for a, b in push_bounds(name):
                segs, n_speech = [], 0
                for i in range(a, b):
                    sg, ns = g.push(f[i:i + 1], lab[i:i + 1])
                    count = sum(g.win_labels)                       # the window this frame's label was decided on
                    seen_counts.add(count)
                    hi_bits.update(k for k in (32, 62) if k < W and g.win_labels[k])
                    o["on_tie"] += int(count == TIE_COUNT.get(name, -1))
                    segs += sg
                    n_speech += ns
                out.append((segs, n_speech))
                n_speech_all += n_speech
                o["segments"] += len(segs)
                o["empty_segments"] += sum(len(x) == 0 for x in segs)
                o["most_in_a_push"] = max(o["most_in_a_push"], len(segs))
                elements += [x.size for x in segs]
                if segs:
                    last_push_segments = len(out) - 1
            if name == "values":
                # which input frames reach a segment: a second run on frames that hold their own index + 1 (0: the zeroed rings)
                gi = make_oracle(c.C, c.N, c.context, c.smoothing_context, c.threshold)
                index = np.repeat(np.arange(1.0, len(lab) + 1.0)[:, None], c.C, axis=1)
                for x in gi.push(index, lab)[0]:
                    rows = x[:, 0].astype(np.int64) - 1
                    emitted.update(np.unique(f[rows[rows >= 0]].view(np.uint64)).tolist())
            frames_all += len(lab)
            per_stream.append(out)
            last.append(last_push_segments)
    o["streams_closing_on_last_run"] = sum(k == max(last) >= 0 for k in last)
    o["bit_32"], o["bit_62"] = 32 in hi_bits, 62 in hi_bits
    o["count_49_of_49"], o["count_48_of_49"] = W == 49 and 49 in seen_counts, W == 49 and 48 in seen_counts
    o["all_speech"], o["no_speech"] = n_speech_all == frames_all, n_speech_all == 0
    o["not_multiple_of_256"] = any(e % THREADS for e in elements)
    o["above_1024"] = any(e > UNROLL * THREADS for e in elements)
    o["above_4096"] = any(e > COLLECT_ROWS * THREADS for e in elements)
    o["special_values_emitted"] = len({int(np.float64(v).view(np.uint64)) for v, _ in SPECIAL} & emitted)
    o["element_counts"] = elements
    return o, per_stream


# ---- replay ---------------------------------------------------------------------------------------------------------------------
def push_inputs(name, k, streams=None):
    """Frames (S, W, C) float64 and labels (S, W) int8 of push k for the case's streams (or the given ones)."""
    c = case(name)
    a, b = push_bounds(name)[k]
    streams = range(c.S) if streams is None else streams
    return np.stack([frames(name, s)[a:b] for s in streams]), np.stack([labels(name, s)[a:b] for s in streams])


def replay(exp: Expected, push):
    """Feed a case, push by push and all streams at once, to push(frames (S, W, C), labels (S, W)) -> (per stream: list of
    segments, per stream: speech frames) and hold it to the fixture: the same number of segments on every push, the same
    lengths, the same speech counts, and rows that equal the float32 casts of the frames the fixture names, bit for bit."""
    c = exp.case
    name = c.name
    for k in range(c.pushes):
        f, lab = push_inputs(name, k)
        segs, n_speech = push(f, lab)
        assert len(segs) == c.S and len(n_speech) == c.S
        for s in range(c.S):
            want = exp.rows_of(s, k)
            assert int(n_speech[s]) == int(exp.speech[s, k]), (name, s, k, "speech frames")
            assert len(segs[s]) == len(want), (name, s, k, "segments closed by this push")
            for e, (got, index) in enumerate(zip(segs[s], want)):
                assert got.dtype == np.float32 and got.shape == (len(index), c.C), (name, s, k, e, got.shape, len(index))
                assert np.array_equal(bits(got), bits(exp.segment(name, s, index))), (name, s, k, e)
