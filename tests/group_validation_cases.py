"""The case table of the group trial-list tests (tests/test_cpu_group_validation.py, tests/test_gpu_group_validation.py): a helper
module like validation_cases.py, no tests in it.

An entry is a group of M models of one size and a trial list in which every trial names its model.  Member k's weights are the
precision tests' decoder / detector (``lstm_reference.decoder_state_dict`` / ``vad_state_dict`` at the member's scale) moved by a
seeded 0.02 x N(0, 1) perturbation, as tests/test_gpu_decoder_group.py::_member_sd does, so no two members are alike; the frames are
N(0, 1) x 2 (``lstm_reference.frames``).  Unless an entry says otherwise its trials lie side by side in one array, in an order that
is neither the list's nor longest-first, and no two trials share a row.

  small, small_17_33   (5, 7) and (17, 33), M = 3: trials of 1 .. 9 frames -- 1 frame, 5 (no multiple of the 4-step chunk), 9
  width_*              (5, 7), M = 3: 300 trials of 1 .. 9 frames (the total selects W = 4) dealt round-robin, in blocks of 100, 199
                       and 1 (a model with a single trial) and of 101, 198 and 1 (every model leaves a partly filled workgroup);
                       140 trials (W = 2) and 6 (W = 1)
  reference            the decoder at (100, 64) x 20 outputs, the detector at (150, 64): M = 3 at scales 1, 4, 1, trials of 1, 5, 37
                       frames for every model, and for the detector one trial of 257 frames
  capacity             M = 64 at (5, 7): one trial of 3 frames for each of 62 models, two models with none
  shared               M = 4, every model lists the same 5 ranges (overlap), the list interleaved by model
  chunked              the decoder's (5, 7) list with ``max_rows`` = 16: sets of 9 + 7 (a trial ending exactly on the cap, behind
                       one longer than half of it), 9 + 1 + 5, 9 + 3 + 4, 2 + 8 + 6

float32 and float64 frames alternate over the entries (``f64``); ``small`` runs with both.  tests/test_cpu_group_validation.py
asserts every condition stated here on the float64 reference alone."""
import collections
import functools

import numpy as np

import lstm_reference as R

O = 20
Entry = collections.namedtuple("Entry", "name H C M scales lengths models f64 max_rows shared")


def _entry(name, H, C, M, lengths, models, f64, scales=None, max_rows=0, shared=False):
    assert len(lengths) == len(models) and all(0 <= m < M for m in models)
    return Entry(name, H, C, M, tuple(scales or (1,) * M), tuple(int(n) for n in lengths), tuple(int(m) for m in models), f64, max_rows, shared)


def _lengths(n, seed):
    """n lengths of 1 .. 9, every value present."""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 10, n)
    v[:9] = rng.permutation(9) + 1
    return v.tolist()


def _blocks(*counts):
    return [m for m, c in enumerate(counts) for _ in range(c)]


SMALL_LENGTHS = [1, 5, 9, 4, 9, 1, 5, 8, 5, 9, 1, 3]
SMALL_MODELS = [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2]
REF_LENGTHS, REF_MODELS = [1, 5, 37, 5, 37, 1, 37, 1, 5], [0, 0, 0, 1, 1, 1, 2, 2, 2]
CHUNK_LENGTHS = [9, 7, 9, 1, 5, 9, 3, 4, 2, 8, 6]
CHUNK_ROWS = 16

COMMON = [
    _entry("small", 5, 7, 3, SMALL_LENGTHS, SMALL_MODELS, False),
    _entry("small_f64", 5, 7, 3, SMALL_LENGTHS, SMALL_MODELS, True),
    _entry("small_17_33", 17, 33, 3, SMALL_LENGTHS, SMALL_MODELS, True),
    _entry("width_round_robin", 5, 7, 3, _lengths(300, 1), [i % 3 for i in range(300)], False),
    _entry("width_100_199_1", 5, 7, 3, _lengths(300, 2), _blocks(100, 199, 1), True),
    _entry("width_101_198_1", 5, 7, 3, _lengths(300, 3), _blocks(101, 198, 1), False),
    _entry("width_140", 5, 7, 3, _lengths(140, 4), [i % 3 for i in range(140)], True),
    _entry("width_6", 5, 7, 3, [9, 1, 5, 2, 8, 3], [0, 1, 2, 2, 1, 0], False),
    _entry("capacity", 5, 7, 64, [3] * 62, [m for m in range(64) if m not in (17, 63)], True),
    _entry("shared", 5, 7, 4, [n for n in (9, 1, 5, 4, 7) for _ in range(4)], [m for _ in range(5) for m in range(4)], False, shared=True),
]
DECODER = COMMON + [
    _entry("reference", 100, 64, 3, REF_LENGTHS, REF_MODELS, False, scales=(1, 4, 1)),
    _entry("chunked", 5, 7, 3, CHUNK_LENGTHS, [i % 3 for i in range(len(CHUNK_LENGTHS))], True, max_rows=CHUNK_ROWS),
]
DETECTOR = COMMON + [
    _entry("reference", 150, 64, 3, REF_LENGTHS + [257], REF_MODELS + [1], False, scales=(1, 4, 1)),
]


# The frames' seeds are chosen, like validation_cases.SEEDS, so that the float64 detector has no near-tie on any frame of any trial
# (|z1 - z0| > 2 x bound): the first shift of an entry's seed at which that holds.  Only the x4 member's 257-frame trial needed one.
SEED_SHIFT = {("reference", 150): 1}


def by_name(table, name):
    return next(e for e in table if e.name == name)


def streams_per_workgroup(n_trials):
    """``dss_dec_streams_per_wg``: the W a list of that many trials runs at."""
    return 1 if 2 * n_trials <= 256 else 2 if n_trials <= 256 else 4


def chunk_sets(lengths, max_rows):
    """The sets of launches ``dss_dec_group_forward_trials_dev`` cuts a list into: consecutive trials while their frames fit."""
    sets, cur = [], []
    for n in lengths:
        if cur and sum(cur) + n > max_rows:
            sets.append(cur)
            cur = []
        cur.append(n)
    return sets + [cur] if cur else sets


def member_sd(kind, H, C, k, scale=1):
    """Weights of member k of a group of decoders (``kind="decoder"``) or detectors (``"vad"``)."""
    import torch
    sd = (R.decoder_state_dict if kind == "decoder" else R.vad_state_dict)(H, C, scale)
    if k:
        g = torch.Generator().manual_seed(4000 + k)
        sd = {n: v + 0.02 * torch.randn(v.shape, generator=g) for n, v in sd.items()}
    return sd


@functools.lru_cache(maxsize=None)
def members(kind, e):
    return [member_sd(kind, e.H, e.C, k, e.scales[k]) for k in range(e.M)]


@functools.lru_cache(maxsize=None)
def layout(e):
    """(frames (N, C) float64 holding float32 values, ranges [(first, len)] in list order).  ``shared`` entries: the distinct
    ranges lie side by side and every model lists each of them."""
    seed = 7000 + sum(ord(c) for c in e.name) + e.H + SEED_SHIFT.get((e.name, e.H), 0)
    if e.shared:
        distinct = list(e.lengths[::e.M])
        owner = [i // e.M for i in range(len(e.lengths))]
    else:
        distinct = list(e.lengths)
        owner = list(range(len(distinct)))
    order = np.random.default_rng(seed).permutation(len(distinct))        # where each distinct trial lies in the array
    first, row = [0] * len(distinct), 0
    for k in order:
        first[k] = row
        row += distinct[k]
    x = R.frames("x2", 1, row, e.C, seed + 1)[0]
    return x, [(first[owner[i]], e.lengths[i]) for i in range(len(e.lengths))]


@functools.lru_cache(maxsize=None)
def reference(kind, e):
    """The float64 model of every trial's own member on it: [(len, O) features] or [(len, 2) logits], in list order."""
    x, ranges = layout(e)
    nets = [R.Net(sd) for sd in members(kind, e)]
    fwd = R.decoder_forward if kind == "decoder" else R.vad_forward
    return [fwd(nets[m], x[None, a:a + n])[0][0] for (a, n), m in zip(ranges, e.models)]


def bound(e, m):
    return R.bound(e.scales[m])


def per_model(e):
    """{m: list positions of model m's trials, in list order}."""
    out = {m: [] for m in range(e.M)}
    for i, m in enumerate(e.models):
        out[m].append(i)
    return out


def offsets(e):
    """First output row of every trial in the concatenated outputs, and the total."""
    return np.concatenate([[0], np.cumsum(e.lengths)]).astype(np.int64)
