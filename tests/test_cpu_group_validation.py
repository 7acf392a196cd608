"""The group trial-list forward calls (Part 17 of include/dss_hip.h) and ``dss_amd.validation.GroupValidationSet`` without a GPU:
the conditions tests/group_validation_cases.py states about its own inputs, held by the float64 reference alone, and the host
paths -- the declared and exported symbols, what the entry points refuse before they touch a device, and the layout of a
validation set.

Which refusals need no device: a NULL group handle, NULL frames or outputs are refused before anything else, so they are tested
here.  A model index out of range and an unloaded member are checked against the group (its M, its members), and a group exists
only on a device: those are tests/test_gpu_group_validation.py's."""
import os
import re

import numpy as np
import pytest

import group_validation_cases as G
import lstm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("dss_vad_group_forward_trials_dev", "dss_dec_group_forward_trials_dev")
TABLES = (("decoder", G.DECODER), ("vad", G.DETECTOR))
ENTRIES = [pytest.param(kind, e, id=f"{kind}-{e.name}") for kind, table in TABLES for e in table]


# ---- the table is what its docstring says ------------------------------------------------------------------------------------------

def test_the_table_holds_the_cases_it_names():
    for kind, table in TABLES:
        names = [e.name for e in table]
        assert len(set(names)) == len(names)
        for e in table:
            assert len(e.lengths) == len(e.models) and min(e.lengths) >= 1 and e.scales == tuple(e.scales) and len(e.scales) == e.M
        for name in ("small", "small_f64", "small_17_33"):
            e = G.by_name(table, name)
            assert e.M == 3 and {1, 5, 9} <= set(e.lengths) <= set(range(1, 10))
            assert all({1, 5, 9} <= {e.lengths[i] for i in p} for p in G.per_model(e).values())
        assert (G.by_name(table, "small").H, G.by_name(table, "small").C) == (5, 7) and not G.by_name(table, "small").f64
        assert G.by_name(table, "small_f64").f64 and G.by_name(table, "small")._replace(name="", f64=True) == G.by_name(table, "small_f64")._replace(name="")
        assert (G.by_name(table, "small_17_33").H, G.by_name(table, "small_17_33").C) == (17, 33)
        for name, counts in (("width_round_robin", [100, 100, 100]), ("width_100_199_1", [100, 199, 1]), ("width_101_198_1", [101, 198, 1])):
            e = G.by_name(table, name)
            assert [len(p) for p in G.per_model(e).values()] == counts and set(e.lengths) == set(range(1, 10))
            assert G.streams_per_workgroup(len(e.lengths)) == 4
        assert all(c % 4 for c in (101, 198, 1)) and 199 % 4 and 1 % 4          # partly filled workgroups at W = 4
        assert G.by_name(table, "width_round_robin").models[:4] == (0, 1, 2, 0)
        assert G.streams_per_workgroup(len(G.by_name(table, "width_140").lengths)) == 2 and len(G.by_name(table, "width_140").lengths) == 140
        assert any(len(p) % 2 for p in G.per_model(G.by_name(table, "width_140")).values())
        assert G.streams_per_workgroup(len(G.by_name(table, "width_6").lengths)) == 1 and len(G.by_name(table, "width_6").lengths) == 6
        cap = G.by_name(table, "capacity")
        assert cap.M == 64 and set(cap.lengths) == {3} and sorted(len(p) for p in G.per_model(cap).values()) == [0, 0] + [1] * 62
        sh = G.by_name(table, "shared")
        _, ranges = G.layout(sh)
        assert sh.M == 4 and len(set(ranges)) == 5 and all(sorted(ranges[i] for i in p) == sorted(set(ranges)) for p in G.per_model(sh).values())
        assert sh.models[:8] == (0, 1, 2, 3, 0, 1, 2, 3)
        ref = G.by_name(table, "reference")
        assert ref.M == 3 and ref.scales == (1, 4, 1) and all({1, 5, 37} <= {ref.lengths[i] for i in p} for p in G.per_model(ref).values())
        assert {e.f64 for e in table} == {False, True}
    assert (G.by_name(G.DECODER, "reference").H, G.by_name(G.DECODER, "reference").C) == (100, 64)
    assert (G.by_name(G.DETECTOR, "reference").H, G.by_name(G.DETECTOR, "reference").C) == (150, 64) and 257 in G.by_name(G.DETECTOR, "reference").lengths
    ch = G.by_name(G.DECODER, "chunked")
    sets = G.chunk_sets(ch.lengths, ch.max_rows)
    assert (ch.H, ch.C, ch.max_rows) == (5, 7, 16) and len(sets) == 4 and all(sum(s) <= 16 for s in sets)
    assert sets[0] == [9, 7] and sum(sets[0]) == 16 and sets[0][0] > 8          # ends exactly on the cap; longer than half of it
    assert G.chunk_sets([3, 3], 0 + 6) == [[3, 3]] and G.chunk_sets([3, 4], 6) == [[3], [4]]


def test_the_width_rule_is_the_library_s():
    src = open(os.path.join(ROOT, "delayed-speech-synthesis_amd", "csrc", "dss_common.h")).read()
    m = re.search(r"dss_dec_streams_per_wg\(int S\) \{ return 2 \* S <= (\d+) \? 1 : \(S <= (\d+) \? 2 : 4\); \}", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (256, 256)
    assert [G.streams_per_workgroup(n) for n in (1, 128, 129, 256, 257)] == [1, 1, 2, 2, 4]


@pytest.mark.parametrize("kind, e", ENTRIES)
def test_trials_do_not_overlap_unless_shared(kind, e):
    x, ranges = G.layout(e)
    assert x.shape[1] == e.C and np.array_equal(x, x.astype(np.float32).astype(np.float64))
    rows = np.zeros(len(x), np.int64)
    for a, n in set(ranges):
        rows[a:a + n] += 1
    assert rows.min() == rows.max() == 1
    assert (len(set(ranges)) < len(ranges)) == e.shared
    order = [a for a, _ in ranges]
    if len(ranges) > 3 and not e.shared:
        assert order != sorted(order)
        assert len(set(e.lengths)) == 1 or order != [a for a, _ in sorted(ranges, key=lambda r: -r[1])]


# ---- the power of the bit and tolerance tests: the wrong model's weights cannot pass ----------------------------------------------------

def _others(e, m):
    """The models a trial of model m is also run on: every other one of a small group, three of a large one."""
    return [k for k in range(e.M) if k != m] if e.M <= 4 else sorted({(m + 1) % e.M, (m - 1) % e.M, 0} - {m})


@pytest.mark.parametrize("kind, e", ENTRIES)
def test_another_model_s_weights_miss_the_bound_on_every_trial(kind, e):
    """On every trial, the float64 outputs of the trial's own model and of any other model of the entry differ by more than twice
    the bound somewhere: a kernel that picks the wrong member's weights cannot pass the float64 test -- nor, a fortiori, the bit
    test against the single-model path.  For ``shared`` these are the trials listed for two different models."""
    x, ranges = G.layout(e)
    nets = [R.Net(sd) for sd in G.members(kind, e)]
    fwd = R.decoder_forward if kind == "decoder" else R.vad_forward
    want = G.reference(kind, e)
    cache = {}
    for i, ((a, n), m) in enumerate(zip(ranges, e.models)):
        for k in _others(e, m):
            if (a, n, k) not in cache:
                cache[(a, n, k)] = fwd(nets[k], x[None, a:a + n])[0][0]
            gap = np.abs(cache[(a, n, k)] - want[i]).max()
            assert gap > 2 * max(G.bound(e, m), G.bound(e, k)), (e.name, i, m, k, gap)


@pytest.mark.parametrize("e", G.DETECTOR, ids=lambda e: e.name)
def test_no_detector_frame_is_a_near_tie(e):
    """|z1 - z0| > 2 x bound on every frame of every trial: a kernel within the bound gives the float64 labels."""
    for i, z in enumerate(G.reference("vad", e)):
        margin = np.abs(z[:, 1] - z[:, 0]).min()
        assert margin > 2 * G.bound(e, e.models[i]), (e.name, i, margin)


# ---- host paths --------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_exported_and_typed():
    import ctypes as C
    from dss_amd import _lib, training, validation
    L = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dss_hip.h")).read(), flags=re.S)
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int
    vp, i, ll = C.c_void_p, C.c_int, C.c_longlong
    assert L.dss_vad_group_forward_trials_dev.argtypes == [vp, vp, i, ll, i, vp, vp, vp, vp, vp, vp]
    assert L.dss_dec_group_forward_trials_dev.argtypes == [vp, vp, i, ll, i, vp, vp, vp, ll, vp, vp]
    for cls in (training.VadGroupTrainerGPU, training.DecoderGroupTrainerGPU):
        assert callable(getattr(cls, "forward_trials_torch"))
    for name in ("GroupValidationSet", "decoder_validation_group", "vad_validation_group"):
        assert hasattr(validation, name), name
    import inspect
    for fn in (training.train_decoders, training.train_vads):
        assert inspect.signature(fn).parameters["group_validation"].default is False


def test_null_arguments_are_refused_without_a_device():
    """The NULL checks precede every device call: a NULL group, and with it any other argument, is refused with a message."""
    from dss_amd import _lib
    L = _lib.load()
    first, length, model = np.zeros(1, np.int64), np.ones(1, np.int32), np.zeros(1, np.int32)
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    rc = L.dss_vad_group_forward_trials_dev(None, p, 0, 1, 1, first.ctypes.data, length.ctypes.data, model.ctypes.data, p, None, None)
    assert rc == -1 and "dss_vad_group_forward_trials_dev: null argument" in L.dss_last_error().decode()
    rc = L.dss_dec_group_forward_trials_dev(None, p, 0, 1, 1, first.ctypes.data, length.ctypes.data, model.ctypes.data, 0, p, None)
    assert rc == -1 and "dss_dec_group_forward_trials_dev: null argument" in L.dss_last_error().decode()


def _corpus(kind, rng, lengths, C=6, n_out=3):
    n = int(sum(lengths))
    ids = np.repeat(np.arange(len(lengths)) % 2, lengths) if len(lengths) else np.zeros(0, np.int64)
    c = dict(hga_activity=rng.standard_normal((n, C)).astype(np.float32), trial_ids=ids)
    if kind == "decoder":
        c["lpc_coefficients"] = rng.standard_normal((n, n_out)).astype(np.float32)
    else:
        c["vad_labels"] = rng.integers(0, 2, n).astype(np.uint8)
    return c


@pytest.mark.parametrize("kind", ("decoder", "vad"))
def test_validation_set_layout_is_the_per_model_trial_bounds(kind):
    """Ranges, models, slices and row counts of a set equal every corpus' own ``trial_bounds``, shifted by the rows in front of it;
    a None corpus and an empty one own nothing; frames and targets are the corpora's, concatenated (with the column gather)."""
    import torch
    from dss_amd.validation import GroupValidationSet, trial_bounds
    rng = np.random.default_rng(5)
    per = [[3, 1, 4], None, [], [2, 2, 5, 1], [7]]
    corpora = [None if n is None else _corpus(kind, rng, n) for n in per]
    corpora[3]["hga_activity"] = corpora[3]["hga_activity"].astype(np.float64)          # one float64 corpus: the set is float64
    cols = [4, 0, 5]
    vs = GroupValidationSet(corpora, kind, columns=cols, device="cpu")
    assert len(vs) == vs.M == 5 and vs.kind == kind
    want_ranges, want_models, row0 = [], [], 0
    for m, c in enumerate(corpora):
        r = [] if c is None else trial_bounds(c["trial_ids"])
        assert [n for _, n in r] == (per[m] or [])
        assert vs.trials[m] == slice(len(want_ranges), len(want_ranges) + len(r))
        assert vs.rows[m] == slice(row0, row0 + sum(n for _, n in r))
        want_ranges += [(row0 + a, n) for a, n in r]
        want_models += [m] * len(r)
        row0 += sum(n for _, n in r)
    assert vs.ranges == want_ranges and vs.models == want_models and vs.n_rows == row0 == 25
    assert vs.lengths.dtype == np.int32 and vs.lengths.tolist() == [n for _, n in want_ranges]
    live = [c for c, n in zip(corpora, per) if n]
    assert vs.frames.dtype == torch.float64 and tuple(vs.frames.shape) == (25, 3)
    assert np.array_equal(vs.frames.numpy(), np.concatenate([np.asarray(c["hga_activity"], np.float64)[:, cols] for c in live]))
    if kind == "decoder":
        assert vs.targets.dtype == torch.float32 and np.array_equal(vs.targets.numpy(), np.concatenate([c["lpc_coefficients"] for c in live]))
    else:
        assert vs.targets.dtype == torch.uint8 and np.array_equal(vs.targets.numpy(), np.concatenate([c["vad_labels"] for c in live]))
    none = GroupValidationSet([None, _corpus(kind, rng, [])], kind, device="cpu")
    assert none.ranges == [] and none.n_rows == 0 and none.frames is None and none.trials == [slice(0, 0)] * 2
    with pytest.raises(ValueError, match="kind"):
        GroupValidationSet([], "gru")
    if kind == "vad":
        bad = _corpus(kind, rng, [2])
        bad["vad_labels"][0] = 2
        with pytest.raises(ValueError, match="0 / 1"):
            GroupValidationSet([bad], kind, device="cpu")
