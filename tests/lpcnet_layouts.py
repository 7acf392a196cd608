"""Structure edges of the CU-resident layout of GRU A for the parity tests (helper module, no tests in it).

Which code of the sample-rate kernels a model runs is decided on the host by build_fast_layout (csrc/dss_lpcnet_model.cpp)
from the 144 per-row-group block counts of GRU A and a handful of limits: DSS_ZRC 12 (10 in the 10-slot layout, 8 on waves
0..3) register slots, DSS_ZR_TAIL 16, DSS_HC 28, DSS_HCX 32, DSS_HX 32, DSS_HBLK_BYTES 151552 and the pair kernel's
DSS_PAIR_HBLK_BYTES 144896.  ``shaped`` builds a model with exactly the block counts asked for, ``CASES`` places one on every
limit and one block past it.  Everything is seeded and generated, nothing is stored.  What a case really reaches is NOT taken
from here: tests/test_cpu_lpcnet_layouts.py asks dss_selftest_fast_layout for every case, and it and
tests/test_gpu_lpcnet_layouts.py take models and inputs from ``CASES`` / ``features`` so that they cannot drift apart.

Pinned columns.  A lane whose list is shorter than its wave's reads on into foreign records and multiplies them by
"column 96", four zeros behind the 96 block columns of the state; so the last real column, 95, next to it matters, and so
does column 0 at the other end.  Every list a case is named for (a register slot list, a tail list, h slots below 28, h
slots 28..31, h slots from 32 on: ``Case.segments``) therefore holds columns 0 and 95, 0 in its first and 95 in its last
slot.  A list of one slot holds 95 alone.  A column stands once in a group's list (but for 'repeated_column'), so a case
names one list per group: the one its edge lies in.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from dss_amd.lpcnet_weights import GRUA_INPUT_FIRST, GRUA_RECUR_FIRST, make_synthetic_weights, pack_blob, synthetic_features
from lpcnet_regimes import GROUPS, join_groups, split_groups

NCOL = 96                                  # block columns of GRU A's state
PAIR_HBLK_BYTES, HBLK_BYTES = 144896, 151552
BASE = (5, 5, 19)                          # blocks per row group of the z, r and h gate unless a case says otherwise
ONE_ZR, ONE_H = 21, 34                     # the row group of the "one group" cases
# The 17 groups of the "heaviest groups" cases.  Both sorts of layout_assign are stable, so equal groups keep their index
# order: the first 16 land on waves 4 / 5, the last one (47) is the heaviest group of waves 0..3.
HEAVY = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 44, 46, 47)
N_ROWS, N_FRAMES = 3, 5                    # two silent frames plus 480 samples: the lists run on every sample


# ---- the builder ------------------------------------------------------------------------------------------------------
def _pin(cols, slot, col):
    """Column ``col`` into ``slot`` of a list; where the list holds it already the two slots swap their columns."""
    where = np.nonzero(cols == col)[0]
    if where.size:
        cols[where[0]] = cols[slot]
    cols[slot] = col


def shaped(w, z=None, r=None, h=None, order="ascending", segments=(), repeat=(), seed=0):
    """Copy of the weight dict ``w`` whose GRU A row groups hold exactly the given block counts (48 ints per gate, None keeps
    the gate).  A shortened group keeps its first blocks; a lengthened one gains blocks drawn like the generator's (normal,
    sigma 0.25 for z and r, 0.2 for h) at columns it does not use yet, seeded per gate and group.  ``order``: every list by
    ascending or by descending column, blocks travelling with their columns.  ``segments`` [(gate, group, lo, hi)] then
    get their pinned columns (module docstring), ``repeat`` [(gate, group, slot, from_slot)] copies a slot's column."""
    w = {k: v.copy() for k, v in w.items()}
    groups = split_groups(w)
    for gate, want in enumerate((z, r, h)):
        for g in range(GROUPS):
            cols, blk = groups[gate * GROUPS + g]
            if want is not None:
                n = int(want[g])
                assert 0 <= n <= NCOL
                if n < len(cols):
                    cols, blk = cols[:n], blk[:n]
                elif n > len(cols):
                    rng = np.random.default_rng([3000 + seed, gate, g])
                    free = np.setdiff1d(np.arange(NCOL), cols // 4)
                    new = rng.choice(free, size=n - len(cols), replace=False)
                    more = (rng.standard_normal((len(new), 4, 8)) * (0.25 if gate < 2 else 0.2)).astype(np.float32)
                    cols = np.concatenate([cols, (new * 4).astype(np.int32)])
                    blk = np.concatenate([blk.reshape(-1, 4, 8), more])
            by = np.argsort(cols, kind="stable")
            if order == "descending":
                by = by[::-1]
            else:
                assert order == "ascending"
            groups[gate * GROUPS + g] = (cols[by].astype(np.int32), blk[by])
    for gate, g, lo, hi in segments:
        cols = groups[gate * GROUPS + g][0]
        assert 0 <= lo < hi <= len(cols), (gate, g, lo, hi, len(cols))
        if hi - lo >= 2:
            _pin(cols, lo, 0)
        _pin(cols, hi - 1, 4 * (NCOL - 1))
    for gate, g, slot, src in repeat:
        cols = groups[gate * GROUPS + g][0]
        cols[slot] = cols[src]
    return join_groups(w, groups)


# ---- the cases --------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    counts: tuple                          # (z, r, h), 48 ints each
    fast_path: int                         # 1 plain, 2 extended paths, 0 generic kernel (RuntimeWarning)
    zr_cap: int                            # register slots per gate on waves 4 / 5
    tail_blocks: int                       # z and r blocks behind their wave's register slots
    pair_fits: bool                        # the two-utterance kernel accepts the model
    segments: tuple = ()                   # (gate, group, lo, hi): the lists the case is named for
    order: str = "ascending"
    repeat: tuple = ()
    gru_a_order: int = GRUA_INPUT_FIRST


def _counts(z=None, r=None, h=None, base=BASE):
    """48 counts per gate from {group: count} dicts (or whole sequences) over the base."""
    out = []
    for gate, spec in enumerate((z, r, h)):
        if spec is None or isinstance(spec, dict):
            c = [base[gate]] * GROUPS
            for g, n in (spec or {}).items():
                c[g] = n
        else:
            c = [int(x) for x in spec]
            assert len(c) == GROUPS
        out.append(tuple(c))
    return tuple(out)


def _heavy(n, last=None):
    """{group: n} for the 17 heavy groups; ``last`` for the 17th where it differs."""
    d = {g: n for g in HEAVY}
    if last is not None:
        d[HEAVY[-1]] = last
    return d


def _capacity(k):
    """h = the first k groups 24, the rest 23 (every list with its pinned columns: one of them is the image's last record)."""
    return _counts(h=[24] * k + [23] * (GROUPS - k)), tuple((2, g, 0, 24 if g < k else 23) for g in range(GROUPS))


# The switch points of the two LDS limits, found by test_cpu_lpcnet_layouts.test_capacity_switch_points stepping k against
# dss_selftest_fast_layout: the image of `_capacity(k)` is 144896 B at k = 12 (= DSS_PAIR_HBLK_BYTES exactly) and 145152 B
# at k = 13; 151424 B at k = 40 and 151680 B at k = 41 (DSS_HBLK_BYTES is 151552).
K_PAIR_LAST, K_LDS_LAST = 12, 40

_W17 = HEAVY[-1]
_rev_zr = [1 + g // 4 for g in range(GROUPS)]
_rev_h = [4 + g // 2 for g in range(GROUPS)]
_over_h = [27] * 33 + [1] * 7 + [0] * 8

CASES = {
    # ---- z / r register slots
    "z10": Case(_counts(z={ONE_ZR: 10}), 1, 10, 0, True, ((0, ONE_ZR, 0, 10),)),
    "z11": Case(_counts(z={ONE_ZR: 11}), 1, 12, 0, True, ((0, ONE_ZR, 0, 11),)),
    "z12_r": Case(_counts(r={ONE_ZR: 12}), 1, 12, 0, True, ((1, ONE_ZR, 0, 12),)),
    # every slot of waves 4 / 5 full in both gates; group 47, the heaviest of waves 0..3, full at 8
    "z12x16": Case(_counts(z=_heavy(12, 8), r=_heavy(12, 8)), 1, 12, 0, True,
                   tuple((gate, g, 0, 8 if g == _W17 else 12) for gate in (0, 1) for g in HEAVY)),
    "z13": Case(_counts(z={ONE_ZR: 13}), 2, 10, 3, False, ((0, ONE_ZR, 10, 13),)),
    "w03_8": Case(_counts(z=_heavy(8), r=_heavy(8)), 1, 10, 0, True, ((0, _W17, 0, 8), (1, _W17, 0, 8))),
    # group 47 on wave 2: 8 register slots and one tail block in each gate; 9 is odd, so wave_nzr = min(10, cap) is clamped
    "w03_9": Case(_counts(z=_heavy(9), r=_heavy(9)), 2, 10, 2, False, ((0, _W17, 8, 9), (1, _W17, 8, 9))),
    # ---- tails
    "tail16_w45": Case(_counts(z={ONE_ZR: 26}), 2, 10, 16, False, ((0, ONE_ZR, 10, 26),)),
    "tail17_w45": Case(_counts(z={ONE_ZR: 27}), 0, 10, 0, False),
    # Corrected from the issue's "17 groups of 24" in both gates: 17 r tails more add 28672 B to the 129936 B image and leave
    # the LDS limit.  z: 16 groups of 10 + 14 on waves 4 / 5 and group 47 with 8 + 16 on wave 2; r: group 47 alone, 8 + 16
    # (tail17_w03 alike with 25)
    "tail16_w03": Case(_counts(z=_heavy(24), r={_W17: 24}, base=(5, 5, 14)), 2, 10, 16 * 14 + 16 + 16, False,
                       ((0, _W17, 8, 24), (1, _W17, 8, 24))),
    "tail17_w03": Case(_counts(z=_heavy(25), r={_W17: 25}, base=(5, 5, 14)), 0, 10, 0, False),
    # ---- h lists
    "h28": Case(_counts(h={ONE_H: 28}), 1, 10, 0, True, ((2, ONE_H, 0, 28),)),
    "h29": Case(_counts(h={ONE_H: 29}), 2, 10, 0, False, ((2, ONE_H, 28, 29),)),
    "h32": Case(_counts(h={ONE_H: 32}), 2, 10, 0, False, ((2, ONE_H, 28, 32),)),
    "h33": Case(_counts(h={ONE_H: 33}), 2, 10, 0, False, ((2, ONE_H, 32, 33),)),
    "h64": Case(_counts(h={ONE_H: 64}, base=(5, 5, 18)), 2, 10, 0, False, ((2, ONE_H, 32, 64),)),
    "h65": Case(_counts(h={ONE_H: 65}, base=(5, 5, 18)), 0, 10, 0, False),
    # ---- image arithmetic
    "h_even": Case(_counts(base=(5, 5, 20)), 1, 10, 0, True, tuple((2, g, 0, 20) for g in range(GROUPS))),
    "h_odd": Case(_counts(base=(5, 5, 21)), 1, 10, 0, True, tuple((2, g, 0, 21) for g in range(GROUPS))),
    "h_none": Case(_counts(base=(5, 5, 0)), 1, 10, 0, True),
    "h_wave_empty": Case(_counts(h={g: 0 for g in (1, 8, 15, 22, 29, 36, 43, 45)}), 1, 10, 0, True),
    # Corrected from the issue's "h = 32 x 20, then 27, 7 x 1, 8 x 0": the h sort is descending, so a lone 27 among 20s is
    # rank 0 and lands on wave 0, and the image's last wave would run 20 slots.  With 27 in the 32 leading groups as well
    # the stable sort leaves group 32 at rank 32: wave 5, the last of the image, runs 28 slots on lists of 27, 1, .., 1, and
    # the last list of the image is read 27 records past its own one (+ 4 fetched ahead); wave 4 holds the empty lists.
    "h_overread": Case(_counts(h=_over_h), 1, 10, 0, True, ((2, 32, 0, 27),) + tuple((2, g, 0, 1) for g in range(33, 40))),
    # ---- capacity
    "pair_last": Case(_capacity(K_PAIR_LAST)[0], 1, 10, 0, True, _capacity(K_PAIR_LAST)[1]),
    "pair_first_over": Case(_capacity(K_PAIR_LAST + 1)[0], 1, 10, 0, False, _capacity(K_PAIR_LAST + 1)[1]),
    "lds_last": Case(_capacity(K_LDS_LAST)[0], 1, 10, 0, False, _capacity(K_LDS_LAST)[1]),
    "lds_first_over": Case(_capacity(K_LDS_LAST + 1)[0], 0, 10, 0, False, _capacity(K_LDS_LAST + 1)[1]),
    # ---- order
    # Corrected from the issue's "counts rise with the group index, both sorts give the reverse permutation": 48 distinct
    # z / r counts would need a 37-block tail.  The counts rise in steps (z, r 1..12 in fours, h 4..27 in twos): the sorts
    # reverse the steps and, being stable, keep the index order inside one.  Every place still gets another group.
    "reversed": Case(_counts(z=_rev_zr, r=_rev_zr, h=_rev_h), 1, 12, 0, True, ((0, 47, 0, 12), (1, 47, 0, 12), (2, 47, 0, 27))),
    "ties": Case(_counts(), 1, 10, 0, True),
    "descending_columns": Case(_counts(), 1, 10, 0, True, order="descending"),
    "repeated_column": Case(_counts(), 1, 10, 0, True, repeat=((0, 9, 3, 1), (1, 30, 4, 0), (2, 17, 11, 2))),
    "z12_order1": Case(_counts(r={ONE_ZR: 12}), 1, 12, 0, True, ((1, ONE_ZR, 0, 12),), gru_a_order=GRUA_RECUR_FIRST),
    "z13_order1": Case(_counts(z={ONE_ZR: 13}), 2, 10, 3, False, ((0, ONE_ZR, 10, 13),), gru_a_order=GRUA_RECUR_FIRST),
}

_built = {}


def build(name):
    """(weight dict, blob) of a named case (cached: both are read-only)."""
    if name not in _built:
        c = CASES[name]
        w = shaped(make_synthetic_weights(0), *c.counts, order=c.order, segments=c.segments, repeat=c.repeat)
        _built[name] = (w, pack_blob(w, gru_a_order=c.gru_a_order))
    return _built[name]


def capacity_blob(k):
    counts, segments = _capacity(k)
    return pack_blob(shaped(make_synthetic_weights(0), *counts, segments=segments))


def features(rows=N_ROWS, frames=N_FRAMES):
    """(rows, frames, 20) inputs shared by all cases: a seeded utterance per row, the second one quiet, the third one loud."""
    f = np.stack([synthetic_features(6100 + b, frames) for b in range(rows)])
    gains = np.array([1.0, 0.05, 3.0], np.float32)
    for b in range(rows):
        f[b, :, :18] *= gains[b % len(gains)]
    return f
