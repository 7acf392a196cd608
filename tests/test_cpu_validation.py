"""Host-side checks of the trial-list validation passes (dss_amd/validation.py, Part 8 of include/dss_hip.h): the trial borders,
the argument checks of the C ABI, the behaviour without a GPU, and the conditions of tests/test_gpu_validation.py on its inputs:
the corpus' and, for the case table of tests/validation_cases.py, the chunk widths the entries claim, no near-tie in any
detector entry, trials that cannot be taken for one another, and the two slips of the trial regressor the table is there to catch."""
import ctypes as C

import numpy as np
import pytest

import lstm_reference as R
import validation_cases as V


def _count_trials(trial_ids):
    """SequentialSpeechTrials._count_trials (local/training.py:61-63)."""
    return len(np.where(trial_ids[:-1] != trial_ids[1:])[0]) + 1


def test_trial_bounds_docstring_example():
    """The example of training.py:69, seq [4, 4, 4, 3, 3, 3, -3, -3, -3, 5, 5, 5, -5, -5, -5, 5, 5, 5]: its borders [0, 3, 6, 9, 12,
    15, 18] make SIX trials (what _count_trials returns for it), and rows 9 .. 12, which that docstring names, are the fourth of
    them (index 3; the docstring's "n=4" counts from one although it says zero-indexed)."""
    from dss_amd.validation import trial_bounds
    seq = np.array([4, 4, 4, 3, 3, 3, -3, -3, -3, 5, 5, 5, -5, -5, -5, 5, 5, 5])
    b = trial_bounds(seq)
    assert len(b) == 6 == _count_trials(seq)
    assert b[4][0] == 12 and b[3] == (9, 3)
    first, length = b[3]
    assert (first, first + length) == (9, 12)
    assert trial_bounds([]) == [] and trial_bounds([7]) == [(0, 1)]


def test_trial_bounds_nine_trials():
    """A list of nine trials of unequal lengths, repeated stimuli negated as prepare_corpus.get_trial_ids writes them (5, -5, 5 are
    three trials): the fourth is rows 9 .. 12 again, every border is where _count_trials counts one."""
    from dss_amd.validation import trial_bounds
    seq = np.repeat([4, 3, -3, 5, -5, 5, 1, -1, 1], [3, 3, 3, 3, 3, 3, 2, 1, 4])
    b = trial_bounds(seq)
    assert len(b) == 9 == _count_trials(seq)
    assert b[3] == (9, 3) and b[8] == (21, 4)
    assert sum(n for _, n in b) == len(seq) and all(b[k][0] + b[k][1] == b[k + 1][0] for k in range(8))


def test_trial_bounds_on_the_session_corpus(golden):
    from dss_amd import session
    from dss_amd.validation import trial_bounds
    g = golden("session.npz")
    trials = [tuple(int(v) for v in t) for t in g["trials"]][1:]
    ids = session.trial_ids(trials, ["ba", "ba", "SILENCE", "du", "du"], ["SILENCE", "ba", "du"], int(g["fs"][0]))
    b = trial_bounds(ids)
    assert len(b) == _count_trials(ids) == 5
    assert [n for _, n in b] == [int(w) for w in g["frame_counts"][1:]]
    assert b[0][0] == 0 and all(b[k][0] + b[k][1] == b[k + 1][0] for k in range(4)) and b[4][0] + b[4][1] == len(ids)


def _check(L, N, ranges, null=None):
    first = np.array([a for a, _ in ranges], np.int64)
    length = np.array([n for _, n in ranges], np.int32)
    total = C.c_longlong(-1)
    args = [first.ctypes.data, length.ctypes.data, C.byref(total)]
    if null is not None:
        args[null] = None
    return L.dss_trials_check(N, len(ranges), *args), total.value


def test_trials_check():
    from dss_amd import _lib
    L = _lib.load()
    assert _check(L, 100, [(50, 50), (0, 100), (10, 1), (10, 1), (99, 1)]) == (0, 153)          # overlapping, unordered, to the last row
    assert _check(L, V.N_ROWS, V.RANGES) == (0, sum(n for _, n in V.RANGES))
    assert _check(L, 100, []) == (0, 0)
    for bad, word in (([(0, 0)], b"frames"), ([(0, -3)], b"frames"), ([(-1, 5)], b"negative"), ([(96, 5)], b"behind"),
                      ([(0, 10), (100, 1)], b"behind"), ([(0, 101)], b"behind")):
        rc, _ = _check(L, 100, bad)
        assert rc == -1 and word in L.dss_last_error(), (bad, L.dss_last_error())
    for null in (0, 1, 2):
        assert _check(L, 100, [(0, 10)], null=null)[0] == -1 and b"null" in L.dss_last_error()
    first = np.zeros(1, np.int64)
    length = np.ones(1, np.int32)
    total = C.c_longlong(0)
    assert L.dss_trials_check(100, -1, first.ctypes.data, length.ctypes.data, C.byref(total)) == -1


def test_no_gpu_raises():
    from dss_amd import _lib
    from dss_amd.validation import decoder_validation, vad_validation
    L = _lib.load()
    if L.dss_device_count() > 0:
        pytest.skip("a GPU is present")
    x = V.corpus(1)[:40]
    ids = np.repeat([1, 2], 20)
    with pytest.raises(_lib.DssError):
        vad_validation(R.vad_state_dict(V.VAD_H, V.C, 1), x, np.zeros(40, bool), ids)
    with pytest.raises(_lib.DssError):
        decoder_validation(R.decoder_state_dict(V.DEC_H, V.C, 1), x, np.zeros((40, 20), np.float32), ids)
    # the reductions take no handle: they fail on their own
    one = np.ones(1, np.int32)
    assert L.dss_vad_score_trials_dev(1, 1, 1, 1, one.ctypes.data, 1, 1, None, None) == -2
    assert L.dss_dec_mse_trials_dev(1, 1, 20, 1, one.ctypes.data, 1, None) == -2


def test_foreign_architecture_is_refused_before_anything_runs():
    """No silent fallback: a state_dict that is not the reference's detector / decoder raises (with or without a GPU)."""
    from dss_amd import _lib
    from dss_amd.validation import decoder_validation, vad_validation
    sd = dict(R.vad_state_dict(V.VAD_H, V.C, 1))
    sd["extra.weight"] = sd["classifier.bias"]
    with pytest.raises((ValueError, _lib.DssError)):
        vad_validation(sd, V.corpus(1)[:8], np.zeros(8, bool), np.ones(8))
    with pytest.raises((ValueError, _lib.DssError)):
        decoder_validation(R.vad_state_dict(V.VAD_H, V.C, 1), V.corpus(1)[:8], np.zeros((8, 20), np.float32), np.ones(8))


@pytest.mark.parametrize("scale", [1, 4])
def test_fixture_has_no_near_tie(scale):
    """The condition under which tests/test_gpu_validation.py may demand equal labels on EVERY frame: on the float64 reference alone,
    no frame of any trial has |z1 - z0| <= 2 x bound(scale) -- zero frames left out."""
    z = V.vad_reference_logits(scale)
    assert z.shape == (sum(n for _, n in V.RANGES), 2)
    margin = np.abs(z[:, 1] - z[:, 0])
    print(f"x{scale}: smallest margin {margin.min():.3e}, 2 x bound {2 * R.bound(scale):.1e}, speech frames {(z[:, 1] > z[:, 0]).mean():.3f}")
    assert int((margin <= 2 * R.bound(scale)).sum()) == 0
    assert sorted({n for _, n in V.RANGES}) == [1, 3, 4, 5, 50, 251, 1500]


# ---- the case table (tests/validation_cases.py): its conditions on the float64 reference alone ---------------------------------------
def test_case_table_constants_are_the_sources():
    """The thresholds, tiles and capacities the table is built around, read from the kernels' sources."""
    src = V.source_constants()
    for name in ("WIDTH_1_UP_TO", "WIDTH_2_UP_TO", "REGRESS_ROWS", "TRIAL_CHUNK", "SCORE_TILE", "MSE_STRIDE"):
        assert getattr(V, name) == src[name], name
    assert (max(e.H for e in V.DETECTOR), max(e.C for e in V.DETECTOR)) == src["VAD_MAX"]
    assert (max(e.H for e in V.DECODER), max(e.C for e in V.DECODER)) == src["DEC_MAX"]
    assert max(e.O for e in V.DECODER) == src["DEC_MAXO"] and {e.O for e in V.DECODER} == {1, 3, 20, 31, 32}
    assert any(2 * e.H % 4 == 2 and e.H > 100 for e in V.DECODER)          # K = 2H = 2 modulo 4 at a large size
    assert {(e.H % 4, e.C % 4) for e in V.DETECTOR} >= {(3, 1), (1, 1), (3, 3), (0, 0)}
    assert V.SCORE_LENGTHS == (1, V.SCORE_TILE - 1, V.SCORE_TILE, V.SCORE_TILE + 1, 2 * V.SCORE_TILE, 2 * V.SCORE_TILE + 1)
    for O in sorted({o for _, o in V.MSE_CASES}):
        counts = sorted(n * o for n, o in V.MSE_CASES if o == O)
        print(f"{O} outputs: elements {counts}")
    counts = {n * o for n, o in V.MSE_CASES}
    assert {V.MSE_STRIDE - 1, V.MSE_STRIDE, V.MSE_STRIDE + 1, 1} <= counts and all(n < 2 * V.MSE_STRIDE for n in counts)
    assert max(max(e.lengths) for e in V.DECODER + V.DETECTOR) <= 513 and max(V.SCORE_LENGTHS) <= 513


def test_case_table_chunks():
    """The chunk arithmetic the decoder entries claim: trials per chunk against the 128 / 256 thresholds, the longest trial of the
    mixed chunk against the regressor's 8-row blocks, the trial counts against the reductions' 256 trials per launch."""
    w, m, r = V.WIDTH, V.MIXED, V.REFERENCE_SIZE
    assert len(w.lengths) == 300 and sorted(set(w.lengths)) == list(range(1, 10)) and w.handles == (300, 256, 129)
    assert [(s, W) for s, _, W in V.decoder_chunks(w.lengths, 300)] == [(300, 4)]
    assert [(s, W) for s, _, W in V.decoder_chunks(w.lengths, 256)] == [(256, 2), (44, 1)]
    assert [(s, W) for s, _, W in V.decoder_chunks(w.lengths, 129)] == [(129, 2), (129, 2), (42, 1)]
    assert len(w.lengths) > V.TRIAL_CHUNK          # two launches of dec_mse_trials_kernel

    assert len(m.lengths) == 140 and sorted(m.lengths)[-4:] == [8, 9, 16, 17] and sorted(m.lengths)[-5] <= 7 and min(m.lengths) == 1
    assert V.decoder_chunks(m.lengths, m.handles[0]) == [(140, 17, 2)] and 17 % V.REGRESS_ROWS
    order = V.longest_first(m.lengths)
    padding, straddling, blocks = V.regress_blocks([m.lengths[i] for i in order])
    print(f"mixed: {blocks} blocks of the regressor, {padding} of pure padding, {straddling} that straddle a trial's end")
    assert padding >= 10 and straddling >= 10 and blocks == (140 * 17 + 7) // 8

    # decoder_validation creates a handle of min(trials, max_streams = 256) streams
    assert len(r.lengths) == 130 and max(r.lengths) == 12 and (r.H, r.C, r.O) == (V.DEC_H, V.C, 20) and r.corpus_form
    assert V.decoder_chunks(r.lengths, min(130, 256)) == [(130, 12, 2)]
    for e in V.DECODER[3:]:
        assert [(s, W) for s, _, W in V.decoder_chunks(e.lengths, e.handles[0])] == [(2, 1)] * 3
    assert all(max(e.lengths) <= V.F64_FRAMES_UP_TO for e in V.DECODER)


@pytest.mark.parametrize("e", V.DECODER, ids=V.dec_ident)
def test_case_table_decoder_trials_are_told_apart(e):
    """Per decoder entry: the list order is neither the longest-first order nor the order of the rows; the trials share no frame;
    and no two trials have equal float64 features on their common frames -- they differ by more than 2 x bound somewhere on
    them, so a trial written to another's rows (an ``out_row`` mix-up) cannot pass, at the float64 bound or bit for bit."""
    sd, x, ranges = V.decoder_inputs(e)
    lengths = [n for _, n in ranges]
    assert tuple(lengths) == e.lengths and x.shape[1] == e.C and tuple(sd["regressor.weight"].shape) == (e.O, 2 * e.H)
    assert V.longest_first(lengths) != list(range(len(lengths)))
    rows = np.zeros(len(x), np.int64)
    for a, n in ranges:
        rows[a:a + n] += 1
    assert (rows == 1).all()
    if not e.corpus_form:
        assert sorted(range(len(ranges)), key=lambda i: ranges[i][0]) not in (list(range(len(ranges))), V.longest_first(lengths))
    f = V.decoder_truth(e)
    assert f.shape == (len(ranges), max(lengths), e.O)
    L = np.asarray(lengths)
    worst = np.inf
    for i in range(len(ranges) - 1):
        common = np.arange(f.shape[1])[None, :] < np.minimum(L[i], L[i + 1:])[:, None]
        d = np.where(common, np.abs(f[i + 1:] - f[i]).max(axis=2), 0.0).max(axis=1)
        worst = min(worst, float(d.min()))
    print(f"{V.dec_ident(e)}: the two most alike trials differ by {worst:.3e} on their common frames (2 x bound {2 * R.bound(e.scale):.1e})")
    assert worst > 2 * R.bound(e.scale)


@pytest.mark.parametrize("e", V.DETECTOR, ids=V.vad_ident)
def test_case_table_detector_has_no_near_tie(e):
    """The condition under which the GPU test may demand the float64 labels on EVERY frame of a detector entry: no frame has
    |z1 - z0| <= 2 x bound(scale), zero frames left out."""
    z = V.detector_truth(e)
    assert z.shape == (sum(e.lengths), 2)
    margin = np.abs(z[:, 1] - z[:, 0])
    print(f"{V.vad_ident(e)}: smallest margin {margin.min():.3e}, 2 x bound {2 * R.bound(e.scale):.1e}, excluded frames "
          f"{int((margin <= 2 * R.bound(e.scale)).sum())}, speech frames {(z[:, 1] > z[:, 0]).mean():.3f}")
    assert int((margin <= 2 * R.bound(e.scale)).sum()) == 0
    assert V.longest_first(list(e.lengths)) != list(range(len(e.lengths)))


def test_case_table_tie_model():
    """The tie model's float64 logits are pairwise equal (so label 0, prob 0.5, loss ln 2 on every frame), and not constant."""
    z = V.detector_truth(V.TIE)
    assert z.shape == (sum(V.TIE.lengths), 2) and np.array_equal(z[:, 0], z[:, 1])
    assert np.ptp(z[:, 0]) > 100 * R.bound(1)
    sd = V.tie_state_dict()
    assert np.array_equal(sd["classifier.weight"][0].numpy(), sd["classifier.weight"][1].numpy())
    assert float(sd["classifier.bias"][0]) == float(sd["classifier.bias"][1])


def test_case_table_score_inputs():
    """What the synthetic logits hold: every kind of frame against both targets in every trial longer than one tile, exp(z - m)
    exactly 0 in float64 on the underflow runs, so that their loss is 0 or the whole gap and prob exactly 0 or 1."""
    z, kind, argmax, runs = V.score_inputs()
    assert z.dtype == np.float32 and z.shape == (sum(V.SCORE_LENGTHS), 2) and np.exp(-2.0 * V.UNDERFLOW) == 0.0
    for s, n in zip(V.bounds_of(V.SCORE_LENGTHS), V.SCORE_LENGTHS):
        if n >= V.SCORE_TILE:
            assert {(int(k), int(t)) for k, t in zip(kind[s], runs[s])} == {(k, t) for k in range(4) for t in (0, 1)}
    ce, p = V.cross_entropy(z, runs), V.softmax_speech(z)
    under = (kind == 1) | (kind == 2)
    assert set(np.unique(ce[under])) == {0.0, 2.0 * V.UNDERFLOW} and set(np.unique(p[under])) == {0.0, 1.0}
    assert np.array_equal(p[kind == 1], np.zeros((kind == 1).sum())) and not argmax[kind == 3].any()
    assert np.abs(ce[kind == 3] - np.log(2.0)).max() <= 1e-14 and np.abs(p[kind == 3] - 0.5).max() <= 1e-15


@pytest.mark.parametrize("defect", ["out_row_in_list_order", "first_padded_row_live"])
def test_power_trial_regressor(defect):
    """A numpy restatement of the trial regressor gives the float64 features of the "mixed" entry; with ``out_row`` taken in list
    order, or with the first padded row of every trial counted as live, it misses them by more than 10 x the bound -- so the
    GPU test at that bound cannot pass a kernel with either defect."""
    e = V.MIXED
    sd, x, ranges = V.decoder_inputs(e)
    lengths = [n for _, n in ranges]
    net = R.Net(sd)
    top = V.decoder_top(net, V._pool(x, ranges), lengths)
    w, b = net.p["regressor.weight"], net.p["regressor.bias"]
    truth = V.decoder_truth(e)
    want = np.concatenate([truth[i, :n] for i, n in enumerate(lengths)])
    assert np.abs(V.regress_trials(top, w, b, lengths, e.handles[0]) - want).max() <= 1e-12
    assert np.abs(V.regress_trials(top, w, b, lengths, 3) - want).max() <= 1e-12          # whatever the chunks
    got = V.regress_trials(top, w, b, lengths, e.handles[0], defect=defect)
    written = ~np.isnan(got).any(axis=1)                   # (rows the defective scatter never reaches are not counted here)
    missed = np.abs(got[written] - want[written]).max(axis=1)
    print(f"{defect}: {int((~written).sum())} of {len(want)} rows not written, {int((missed > R.bound(e.scale)).sum())} written rows miss, "
          f"the worst by {missed.max():.3e} (10 x bound {10 * R.bound(e.scale):.0e})")
    assert missed.max() > 10 * R.bound(e.scale)
