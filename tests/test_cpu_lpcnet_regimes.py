"""CPU proof that the models of tests/lpcnet_regimes.py reach the value regimes they are named after, on the oracle alone
and for every input tests/test_gpu_lpcnet_regimes.py feeds the kernels: witness counters of oracle/lpcnet_oracle.c
(clamped table indices, saturated results, subnormal arguments, extreme excitation indices, int16 clips, decided and
equal tree-walk comparisons), finiteness, determinism, and -- for 'tiny' -- the oracle with FTZ + DAZ switched on, which
IS the subtly wrong kernel and fails the comparison with its own unflushed run.

Minimum counts are conditions: at least MIN_COUNT occurrences per utterance, and the fractions named in each test.  Run
with -rP to see every count next to its minimum.

One witness the regimes were specified with cannot exist, and the file says so instead of asserting it: "activation
results outside [-1, 1] beyond the table".  tansig_table holds tanh(0.04 i) rounded to 6 decimals, which is exactly 1.0 for
i >= 191; there dy = 1 - y*y is exactly 0 and tanh_approx returns exactly +-1 whatever the distance from the table's end
(test_table_ends_are_exactly_one proves it over a dense sweep and at every clamped argument the 'hot' runs meet).  For the
same reason "index clamp 199 instead of 200" and "correction dropped after the clamp" are EQUIVALENT mutants of the helper,
not wrong kernels; the mutants that do change values (clamp at 189, sign lost after the clamp) are the ones asserted to
differ.  The count that replaces it is `saturated`: results that are exactly +-1."""
import ctypes

import numpy as np
import pytest

import lpcnet_regimes as R
from dss_amd import _lib
from dss_amd.lpcnet_weights import GRUA_RECUR_FIRST, pack_blob, synthetic_blob, unpack_blob

MIN_COUNT = 100            # occurrences per utterance of every clamp / saturation / extreme-index / clip witness
MIN_FRACTION = 0.01        # of GRU A's gate evaluations at the clamp ('hot'); of the forced logits that flushing changes ('tiny')


@pytest.fixture(scope="module")
def orc(oracle):
    try:
        oracle.require_witnesses()
    except RuntimeError as e:
        pytest.fail(str(e))
    return oracle


@pytest.fixture(scope="module")
def table(orc):
    return orc.lpcnet_table(orc.lpcnet_model(synthetic_blob(0)), 1, 256)


def _free_run(orc, m, feats, clamp_cap=0):
    F = feats.shape[0]
    dec = orc.decoder(m, trace_cap=F * 160, count=True, clamp_cap=clamp_cap)
    pcm = np.concatenate([dec.synthesize(feats[t]) for t in range(F)])
    return pcm, dec


def _forced_run(orc, m, feats, exc):
    F = feats.shape[0]
    dec = orc.decoder(m, trace_cap=F * 160, count=True)
    dec.force(exc[320:])
    pcm = np.concatenate([dec.synthesize(feats[t]) for t in range(F)])
    return pcm, dec


def _check(label, value, minimum):
    print(f"  {label}: {value} (minimum {minimum})")
    assert value >= minimum, (label, value, minimum)


def _layout(blob):
    info = (ctypes.c_int * 8)()
    L = _lib.load()
    assert L.dss_selftest_fast_layout(blob, len(blob), info) == 0, L.dss_last_error().decode()
    return dict(zip(("fast_path", "zr_max", "h_max", "lds_bytes", "zr_cap", "tail_blocks", "mismatches", "oob"), list(info)))


# ---- the helper at and beyond the ends of its table ----------------------------------------------------------------
def _tanh_np(tab, x, clamp=200, keep_sign=True):
    """numpy restatement of tanh_approx (float32 throughout, the index through double like the C source)."""
    x = np.asarray(x, np.float32)
    sign = np.where(x < 0, np.float32(-1), np.float32(1))
    a = np.abs(x)
    i = np.floor((np.float32(.5) + np.float32(25) * a).astype(np.float64)).astype(np.int64)
    clamped = i > clamp
    i = np.clip(i, 0, clamp)
    a = a - np.float32(.04) * i.astype(np.float32)
    y = tab[i]
    dy = np.float32(1) - y * y
    y = y + a * dy * (np.float32(1) - y * a)
    if not keep_sign:
        sign = np.where(clamped, np.float32(1), sign)
    return (sign * y).astype(np.float32)


def test_table_ends_are_exactly_one(orc):
    m = orc.lpcnet_model(synthetic_blob(0))
    tab = orc.lpcnet_table(m, 0, 201)
    assert (tab[191:] == 1.0).all() and (tab[:191] < 1.0).all()
    rng = np.random.default_rng(3)
    xs = np.concatenate([rng.uniform(-9, 9, 4000), rng.uniform(-1e6, 1e6, 500), [0.0, -0.0, 7.98, 8.0, 8.02, 1e-40, -3e-39, 8e7]])
    xs = xs.astype(np.float32)
    want = np.array([orc.lib.oracle_tanh_approx(m, float(x)) for x in xs], np.float32)
    assert np.array_equal(_tanh_np(tab, xs), want)                       # the restatement is the oracle's helper
    dense = np.concatenate([np.linspace(0, 8.5, 4_000_001), np.geomspace(8.5, 8e7, 200_001)]).astype(np.float32)
    r = _tanh_np(tab, dense)
    assert np.abs(r).max() == 1.0 and (r[dense >= 7.62] == 1.0).all()    # never outside [-1, 1]; exactly 1 from index 191 on
    tiny_x = np.array([1e-45, 1e-40, -5e-39, 1.1e-38], np.float32)
    assert np.array_equal(_tanh_np(tab, tiny_x), tiny_x)                 # first cell: the argument itself, subnormals kept


# ---- every input of the GPU file: finite, deterministic -----------------------------------------------------------
@pytest.mark.parametrize("name,order", [(n, 0) for n in R.CASES] + [(n, GRUA_RECUR_FIRST) for n in R.ORDER1_CASES])
def test_every_gpu_input_is_finite_and_deterministic(orc, table, name, order):
    _, blob = R.build(name, table, gru_a_order=order)
    m = orc.lpcnet_model(blob)
    feats = R.features(name)
    exc = R.forced_excitation(3, feats.shape[1])
    print(f"{name} (gru_a_order {order})")
    for b in range(feats.shape[0]):
        pcm, dec = _free_run(orc, m, feats[b])
        c = dec.counters
        pcm2, dec2 = _free_run(orc, m, feats[b])
        assert np.array_equal(pcm, pcm2) and np.array_equal(dec.trace_pcm, dec2.trace_pcm), (name, b, "not deterministic")
        n = (feats.shape[1] - 2) * 160
        assert c.n_pre == n and np.isfinite(dec.trace_pcm).all()
        print(f"  row {b}: non-finite {c.nonfinite} (maximum 0), pre-quantised value in [{c.pre_min:.6g}, {c.pre_max:.6g}]")
        assert c.nonfinite == 0, (name, b)
        for which, width in ((0, 1152), (1, 48), (2, 16), (3, 384), (4, 16)):
            assert np.isfinite(dec.tap(which, width)).all()
        if b < 3:
            _, fdec = _forced_run(orc, m, feats[b], exc[b])
            assert fdec.counters.nonfinite == 0 and np.isfinite(fdec.forced_logits).all(), (name, b, "forced")
            assert np.isfinite(fdec.trace_pcm).all()


# ---- hot -------------------------------------------------------------------------------------------------------------
def test_hot_reaches_the_clamp_in_both_grus(orc, table):
    """Per utterance: >= MIN_COUNT clamped gate arguments in GRU A and in GRU B, >= 1 % of GRU A's evaluations at the clamp,
    >= MIN_COUNT results exactly +-1 in each; no result outside [-1, 1] (none can exist, module docstring).  Power, on the
    clamped arguments themselves: a helper that clamps at 189, or loses the sign after the clamp, gives other values;
    clamping at 199 or dropping the correction after the clamp gives the same ones (equivalent on this table)."""
    _, blob = R.build("hot", table)
    m = orc.lpcnet_model(blob)
    tab = orc.lpcnet_table(m, 0, 201)
    feats = R.features("hot")
    for b in range(feats.shape[0]):
        _, dec = _free_run(orc, m, feats[b], clamp_cap=1 << 20)
        c = dec.counters
        print(f"hot row {b}")
        _check("GRU A arguments beyond the table", c.site("clamped", "gru_a"), MIN_COUNT)
        _check("GRU A clamped / evaluated", round(c.site("clamped", "gru_a") / c.site("evals", "gru_a"), 4), MIN_FRACTION)
        _check("GRU B arguments beyond the table", c.site("clamped", "gru_b"), MIN_COUNT)
        _check("GRU A results exactly +-1", c.site("saturated", "gru_a"), MIN_COUNT)
        _check("GRU B results exactly +-1", c.site("saturated", "gru_b"), MIN_COUNT)
        _check("dual-FC arguments beyond the table", c.site("clamped", "dual_fc"), MIN_COUNT)
        print(f"  results outside [-1, 1]: {sum(c.out_of_range)} (none can exist)")
        assert sum(c.out_of_range) == 0
        x = dec.clamp_x[:c.clamp_n]
        assert c.clamp_n >= 2 * MIN_COUNT and np.abs(x).max() < 2.0 ** 31 / 25 and (np.abs(x) > 8).all()
        _check("largest clamped |argument|", float(np.abs(x).max()), 1e4)
        good = _tanh_np(tab, x)
        assert (np.abs(good) == 1.0).all() and (good < 0).sum() >= MIN_COUNT and (good > 0).sum() >= MIN_COUNT
        assert not np.array_equal(_tanh_np(tab, x, clamp=189), good)
        assert (_tanh_np(tab, x, clamp=189) != good).sum() >= MIN_COUNT
        assert (_tanh_np(tab, x, keep_sign=False) != good).sum() >= MIN_COUNT
        assert np.array_equal(_tanh_np(tab, x, clamp=199), good)            # equivalent mutant: table[199] == table[200] == 1
        assert np.array_equal(np.sign(x).astype(np.float32) * tab[200], good)   # ... and so is "no correction after the clamp"


# ---- peaked ----------------------------------------------------------------------------------------------------------
def test_peaked_samples_both_ends_and_clips(orc, table):
    """Per utterance, free running: excitation index 0 and 255 each >= MIN_COUNT times, PCM at +32767 and at -32767 (the
    oracle clips to -32767, not -32768) each >= MIN_COUNT times, tree-walk logits beyond either end of the threshold table
    each >= MIN_COUNT times, and the comparison `threshold < logit` taken at equality at least once (the builder puts table
    entries themselves into the root's and the last level's logits; a draw hits a given entry once in 256).  Teacher
    forced: logits above the largest and below the smallest threshold, and logits equal to a table entry, in every sample."""
    _, blob = R.build("peaked", table)
    m = orc.lpcnet_model(blob)
    feats = R.features("peaked")
    exc = R.forced_excitation(3, feats.shape[1])
    for b in range(feats.shape[0]):
        pcm, dec = _free_run(orc, m, feats[b])
        c = dec.counters
        print(f"peaked row {b}")
        _check("excitation index 0", c.exc_hist[0], MIN_COUNT)
        _check("excitation index 255", c.exc_hist[255], MIN_COUNT)
        _check("PCM == +32767", int((pcm == 32767).sum()), MIN_COUNT)
        _check("PCM == -32767", int((pcm == -32767).sum()), MIN_COUNT)
        assert c.clip_hi <= (pcm == 32767).sum() and c.clip_lo <= (pcm == -32767).sum()
        assert pcm.min() == -32767
        _check("walk logits above the table", c.walk_above, MIN_COUNT)
        _check("walk logits below the table", c.walk_below, MIN_COUNT)
        _check("walk comparisons at equality", c.walk_equal, 1)
        _check("pre-quantised |value| maximum", max(-c.pre_min, c.pre_max), 32768.0)
        if b < 3:
            _, fdec = _forced_run(orc, m, feats[b], exc[b])
            lo = fdec.forced_logits[:, 1:]
            _check("forced logits above the table", int((lo > table[255]).sum()), MIN_COUNT)
            _check("forced logits below the table", int((lo < table[0]).sum()), MIN_COUNT)
            _check("forced logits equal to a table entry", int(np.isin(lo, table).sum()), MIN_COUNT)
            assert (np.isin(lo, table).sum(axis=1) > 0).all()


# ---- tiny ------------------------------------------------------------------------------------------------------------
def test_tiny_depends_on_subnormals(orc, table):
    """Per utterance: >= MIN_COUNT subnormal gate arguments in GRU A, and the oracle with FTZ + DAZ gives other
    teacher-forced logits in >= 1 % of all node logits; its free-running PCM differs for at least one utterance (here: all).
    The flushed oracle is the wrong kernel this regime exists to catch: it fails the very comparison the GPU has to pass."""
    _, blob = R.build("tiny", table)
    _, w = unpack_blob(blob)
    tiny32 = np.finfo(np.float32).tiny
    stored = sum(int(((np.abs(w[k]) < tiny32) & (w[k] != 0)).sum()) for k in ("embed_sig", "embed_pred", "embed_exc", "gru_a_w", "dual_fc_w"))
    _check("stored subnormal weights", stored, MIN_COUNT)
    m = orc.lpcnet_model(blob)
    feats = R.features("tiny")
    exc = R.forced_excitation(3, feats.shape[1])
    try:
        with orc.flush_denormals():
            pass
    except NotImplementedError as e:
        pytest.skip(f"subnormal witness not available: {e}")
    pcm_rows_differ = 0
    for b in range(feats.shape[0]):
        pcm, dec = _free_run(orc, m, feats[b])
        print(f"tiny row {b}")
        _check("GRU A subnormal gate arguments", dec.counters.site("subnormal_in", "gru_a"), MIN_COUNT)
        assert orc.lib.oracle_get_flush_denormals() == 0
        with orc.flush_denormals():
            assert orc.lib.oracle_get_flush_denormals() == 3
            pcm_f, _ = _free_run(orc, m, feats[b])
        assert orc.lib.oracle_get_flush_denormals() == 0                  # mode restored
        d = int((pcm_f != pcm).sum())
        print(f"  PCM samples that differ flushed / unflushed: {d} of {pcm.size}")
        pcm_rows_differ += d > 0
        if b < 3:
            _, fdec = _forced_run(orc, m, feats[b], exc[b])
            with orc.flush_denormals():
                _, fdec_f = _forced_run(orc, m, feats[b], exc[b])
            lo, lo_f = fdec.forced_logits[:, 1:], fdec_f.forced_logits[:, 1:]
            _check("forced logits that differ flushed / unflushed, fraction", round(float((lo != lo_f).mean()), 4), MIN_FRACTION)
            assert not np.array_equal(lo, lo_f)                              # the flushed oracle fails the comparison
    _check("utterances whose PCM differs flushed / unflushed", pcm_rows_differ, 1)


# ---- empty -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["empty", "empty_gate", "empty_skewed"])
def test_empty_row_groups_are_in_the_blob(orc, table, name):
    """From the packed blob: which row groups have no block (three per gate; with 'empty_gate' all 48 of the z gate), that
    0.0 and -0.0 weights survive pack_blob -> unpack_blob bit for bit, and what the loader's layout builder makes of it."""
    w, blob = R.build(name, table)
    dims, back = unpack_blob(blob)
    assert pack_blob(back, dims) == blob
    for k in w:
        assert np.array_equal(w[k].view(np.uint32) if w[k].dtype == np.float32 else w[k], back[k].view(np.uint32) if back[k].dtype == np.float32 else back[k]), k
    bits = back["gru_a_w"].view(np.uint32)
    pos0, neg0 = int((bits == 0).sum()), int((bits == 0x80000000).sum())
    print(f"{name}: weights +0.0: {pos0}, -0.0: {neg0} (minimum {MIN_COUNT} each)")
    assert pos0 >= MIN_COUNT and neg0 >= MIN_COUNT
    cnt = R.group_counts(back)
    for gate in range(3):
        for g in R.EMPTY_GROUPS[gate]:
            assert cnt[gate, g] == 0, (gate, g)
    if name == "empty_gate":
        assert (cnt[0] == 0).all() and cnt[1].sum() > 0 and cnt[2].sum() > 0
    assert cnt.sum() == back["gru_a_w"].shape[0]
    info = _layout(blob)
    print(f"{name}: empty groups per gate {[int((cnt[g] == 0).sum()) for g in range(3)]}, layout {info}")
    assert info["fast_path"] == R.CASES[name] and info["mismatches"] == 0 and info["oob"] == 0, info


@pytest.mark.parametrize("name", [n for n in R.CASES if not n.startswith("empty")])
def test_kernel_choice_of_the_other_cases(orc, table, name):
    info = _layout(R.build(name, table)[1])
    assert info["fast_path"] == R.CASES[name] and info["mismatches"] == 0 and info["oob"] == 0, info


def test_a_stale_oracle_library_is_named(orc):
    import oracle_api
    stale = object.__new__(oracle_api.Oracle)
    stale.lib, stale.has_witnesses = orc.lib, False
    with pytest.raises(RuntimeError, match="rebuild oracle/"):
        stale.require_witnesses()
    with pytest.raises(RuntimeError, match="rebuild oracle/"):
        stale.decoder(None, count=True)
