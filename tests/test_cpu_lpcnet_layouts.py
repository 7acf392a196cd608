"""CPU proof that the models of tests/lpcnet_layouts.py sit on the capacity edges they are named after: the block counts are
the table's, dss_selftest_fast_layout (which walks the layout as the kernels index it) finds every block in its place and
no read outside the image, and reports the kernel choice, register capacity, tail blocks and image size the table claims;
the lists a case is named for hold columns 0 and 95; and the oracle runs the inputs of tests/test_gpu_lpcnet_layouts.py
finite.  A case that does not reach its edge fails here, not silently on the GPU.  Run with -rP to see the library's
figures per case."""
import ctypes

import numpy as np
import pytest

import lpcnet_layouts as Y
import lpcnet_regimes as R
from dss_amd import _lib
from dss_amd.lpcnet_weights import unpack_blob

KEYS = ("fast_path", "zr_max", "h_max", "lds_bytes", "zr_cap", "tail_blocks", "mismatches", "oob")


def _layout(blob):
    info = (ctypes.c_int * 8)()
    L = _lib.load()
    assert L.dss_selftest_fast_layout(blob, len(blob), info) == 0, L.dss_last_error().decode()
    return dict(zip(KEYS, list(info)))


@pytest.mark.parametrize("name", list(Y.CASES))
def test_case_reaches_its_edge(name):
    c = Y.CASES[name]
    w, blob = Y.build(name)
    dims, back = unpack_blob(blob)
    cnt = R.group_counts(back)
    assert np.array_equal(cnt, np.array(c.counts)), name
    assert cnt.sum() == back["gru_a_w"].shape[0]
    info = _layout(blob)
    print(f"{name}: {info}")
    assert info["mismatches"] == 0 and info["oob"] == 0, info
    assert (info["fast_path"], info["zr_cap"], info["tail_blocks"]) == (c.fast_path, c.zr_cap, c.tail_blocks), info
    assert info["zr_max"] == max(max(c.counts[0]), max(c.counts[1])) and info["h_max"] == max(c.counts[2])
    if info["fast_path"]:
        assert info["lds_bytes"] <= Y.HBLK_BYTES
        # the pair kernel takes plain layouts up to its own limit (dss_pair_fits)
        assert c.pair_fits == (info["fast_path"] == 1 and info["lds_bytes"] <= Y.PAIR_HBLK_BYTES), info
    else:
        assert not c.pair_fits
    # the lists the case is named for: column 0 first and column 95 last (95 alone in a list of one slot)
    groups = R.split_groups(back)
    for gate, g, lo, hi in c.segments:
        cols = groups[gate * R.GROUPS + g][0] // 4
        assert cols[hi - 1] == Y.NCOL - 1 and (hi - lo < 2 or cols[lo] == 0), (name, gate, g, lo, hi, cols)
    for gate in range(3):
        for g in range(R.GROUPS):
            cols = groups[gate * R.GROUPS + g][0] // 4
            dup = len(cols) - len(set(cols.tolist()))
            assert dup == sum(1 for rg, rgrp, _, _ in c.repeat if (rg, rgrp) == (gate, g)), (name, gate, g)
            if c.order == "descending" and len(cols) > 1:
                assert (np.diff(cols) < 0).all()


def test_the_edges_differ_from_their_neighbours():
    """What the case names promise about each other: one more block changes the capacity, the kernel or the image."""
    lay = {n: _layout(Y.build(n)[1]) for n in ("z10", "z11", "z13", "w03_8", "w03_9", "h28", "h29", "h_even", "h_odd", "h_none",
                                               "h_overread", "h_wave_empty", "ties")}
    assert lay["z10"]["zr_cap"] == 10 and lay["z11"]["zr_cap"] == 12 and lay["z13"]["zr_cap"] == 10
    assert lay["w03_8"]["fast_path"] == 1 and lay["w03_9"]["fast_path"] == 2
    assert lay["h28"]["fast_path"] == 1 and lay["h29"]["fast_path"] == 2
    # 48 x 20 records and a spare one between all groups of a wave (42); 48 x 21 records and none; + 4 fetched ahead
    assert lay["h_even"]["lds_bytes"] == (48 * 20 + 42 + 4) * 128
    assert lay["h_odd"]["lds_bytes"] == (48 * 21 + 4) * 128 + 128       # wave_nh is 22: the last list over-reads one record
    assert lay["h_none"]["lds_bytes"] == (42 + 4) * 128                  # no record but the spares and the look-ahead
    # waves 0..3: 32 lists of 27, no spare record (odd).  Wave 4: eight empty lists, a spare record between them (7).  Wave 5,
    # the last of the image: lists of 27, 1, .., 1, each an odd number of records after the one before, so no spare; it runs
    # 28 slots, and its last list, one record at 864 + 7 + 27 + 6, is read to 28 + 4 records from its start
    assert lay["h_overread"]["lds_bytes"] == (32 * 27 + 7 + 27 + 6 + 28 + 4) * 128
    # 40 lists of 19 and the empty wave's 7 spare records; the last list is read to 20 + 4 records from its start
    assert lay["h_wave_empty"]["lds_bytes"] == (40 * 19 + 7 - 19 + 20 + 4) * 128


def test_capacity_switch_points():
    """h = k groups of 24, the rest 23, k stepped from 0 to 48: the image grows with k, the pair kernel's limit and the LDS
    limit are each crossed once, at the k the table's cases are built with."""
    rows = [_layout(Y.capacity_blob(k)) for k in range(R.GROUPS + 1)]
    size = [r["lds_bytes"] for r in rows]
    assert all(a <= b for a, b in zip(size, size[1:]))
    pair = [r["fast_path"] == 1 and r["lds_bytes"] <= Y.PAIR_HBLK_BYTES for r in rows]
    fast = [r["fast_path"] == 1 for r in rows]
    k_pair, k_lds = max(k for k, ok in enumerate(pair) if ok), max(k for k, ok in enumerate(fast) if ok)
    print(f"pair kernel: k = {k_pair} -> {size[k_pair]} B, k = {k_pair + 1} -> {size[k_pair + 1]} B (limit {Y.PAIR_HBLK_BYTES})")
    print(f"LDS: k = {k_lds} -> {size[k_lds]} B, k = {k_lds + 1} -> {size[k_lds + 1]} B (limit {Y.HBLK_BYTES})")
    assert all(pair[:k_pair + 1]) and not any(pair[k_pair + 1:])
    assert all(fast[:k_lds + 1]) and not any(fast[k_lds + 1:])
    assert (k_pair, k_lds) == (Y.K_PAIR_LAST, Y.K_LDS_LAST)
    assert size[k_pair] == Y.PAIR_HBLK_BYTES                                   # k = 12 fills the pair limit exactly
    assert size[k_lds] <= Y.HBLK_BYTES < size[k_lds + 1]
    for name, k in (("pair_last", k_pair), ("pair_first_over", k_pair + 1), ("lds_last", k_lds), ("lds_first_over", k_lds + 1)):
        assert Y.build(name)[1] == Y.capacity_blob(k), name


@pytest.mark.parametrize("name", list(Y.CASES))
def test_every_gpu_input_is_finite(oracle, name):
    """Free running: the PCM is not all zero after the two silent frames; teacher forced: every node logit is finite."""
    m = oracle.lpcnet_model(Y.build(name)[1])
    feats = Y.features()
    B, F = feats.shape[:2]
    exc = R.forced_excitation(B, F)
    for b in range(B):
        dec = oracle.decoder(m, trace_cap=F * 160)
        pcm = np.concatenate([dec.synthesize(feats[b, t]) for t in range(F)])
        assert (pcm[:320] == 0).all() and pcm[320:].any(), (name, b)
        assert np.isfinite(dec.trace_pcm[:(F - 2) * 160]).all(), (name, b)
        fdec = oracle.decoder(m, trace_cap=F * 160)
        fdec.force(exc[b, 320:])
        for t in range(F):
            fdec.synthesize(feats[b, t])
        assert fdec.forced_logits.shape == ((F - 2) * 160, 256) and np.isfinite(fdec.forced_logits).all(), (name, b)
