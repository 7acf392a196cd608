"""CPU half of the trainers' case table (tests/training_cases.py; tests/test_gpu_training_cases.py runs the kernels over it): the
table is well-posed -- on every entry torch float32 CPU autograd alone stays within a quarter of the GPU tests' bound, so that
bound keeps its meaning (4 x torch float32's own error) on the new inputs; the written-out references agree with autograd there;
the injected defects still exceed ten bounds at the odd sizes; the decoder's ``case_inputs`` has not moved the existing cases; and
the table contains what it is there for."""
import hashlib
import os
import re

import numpy as np
import pytest

import lstm_reference as R
import decoder_training_reference as D
import vad_training_reference as V
import training_cases as TC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "delayed-speech-synthesis_amd", "csrc")


def _smallest(table, n=3):
    return sorted(table, key=lambda e: e.T * (e.H + e.C))[:n]


# ---- the condition the table is held to ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("run", TC.runs(TC.DECODER) + TC.runs(TC.DETECTOR), ids=TC.run_id)
def test_torch_float32_alone_stays_within_a_quarter_of_the_bound(run):
    e, mask = run
    bound = (V if e.O is None else D).GRAD_BOUND
    err, k = TC.float32_error(e, mask)
    print(f"{'detector' if e.O is None else 'decoder'} {TC.run_id(run)}: torch float32 worst tensor {k} {err[k]:.3g} (limit {bound / 4:.3g})")
    assert all(np.isfinite(v) for v in err.values())
    assert err[k] <= bound / 4, (run, k, err[k])


def test_both_bounds_are_the_ones_the_table_was_measured_against():
    assert D.GRAD_BOUND == 6e-6 and V.GRAD_BOUND == 6e-6


# ---- the written-out references at the new sizes ---------------------------------------------------------------------------

@pytest.mark.parametrize("run", TC.runs(_smallest(TC.DECODER)), ids=TC.run_id)
def test_written_out_trial_is_autograd(run):
    sd, x, y, m = TC.decoder_inputs(*run)
    l0, g0, f0 = TC.decoder_truth(*run)
    l1, g1, f1 = D.manual_trial(sd, x, y, m)
    assert abs(l0 - l1) <= 1e-12
    for k in D.KEYS:
        assert np.abs(g0[k] - g1[k]).max() <= 1e-12 * max(1.0, np.abs(g0[k]).max()), k
    assert np.abs(f0 - f1).max() <= 1e-12


@pytest.mark.parametrize("run", TC.runs(_smallest(TC.DETECTOR)), ids=TC.run_id)
def test_written_out_window_is_autograd(run):
    sd, x, y, state, m = TC.detector_inputs(*run)
    l0, g0, (h0, c0) = TC.detector_truth(*run)
    l1, g1, (h1, c1) = V.manual_window(sd, x, y, state, m, max_window=run[0].T)
    assert abs(l0 - l1) <= 1e-12
    for k in V.KEYS:
        assert np.abs(g0[k] - g1[k]).max() <= 1e-12 * max(1.0, np.abs(g0[k]).max()), k
    assert np.abs(h0 - h1).max() <= 1e-12 and np.abs(c0 - c1).max() <= 1e-12


def test_the_three_smallest_are_the_odd_and_the_one_unit_entries():
    assert [TC.ident(e) for e in _smallest(TC.DECODER)] == ["1-1-3-1-20", "6-5-8-1-1", "7-5-9-1-20"]
    assert [TC.ident(e) for e in _smallest(TC.DETECTOR)] == ["1-1-3-1", "7-5-9-1", "33-17-17-1"]


# ---- power at the odd sizes -------------------------------------------------------------------------------------------------
# Left out, because they cannot show: the two mask defects without a mask (there is no mask to forget or to swap), and the
# detector's divisor_max_window at every entry: the table's trainers have max_window = T, so dividing by it is dividing by T.
MASK_DEFECTS = ("mask_not_in_backward", "mask_halves_swapped")
DETECTOR_CANNOT_SHOW = ("divisor_max_window",)


def _defect_runs(defects):
    return [(d, mask) for d in defects for mask in (None, "random") if not (mask is None and d in MASK_DEFECTS)]


@pytest.mark.parametrize("defect, mask", _defect_runs(D.DEFECTS))
def test_each_decoder_defect_exceeds_ten_bounds_at_7_5_9(defect, mask):
    e = TC.DECODER[0]
    assert TC.case(e) == (7, 5, 9, 1)
    sd, x, y, m = TC.decoder_inputs(e, mask)
    want = D.manual_trial(sd, x, y, m)[1]
    worst = max(D.rel_errors(D.manual_trial(sd, x, y, m, defect=defect)[1], want).values())
    print(defect, mask, worst)
    assert worst > 10 * D.GRAD_BOUND


@pytest.mark.parametrize("defect, mask", _defect_runs([d for d in V.DEFECTS if d not in DETECTOR_CANNOT_SHOW]))
def test_each_detector_defect_exceeds_ten_bounds_at_7_5_9(defect, mask):
    e = TC.DETECTOR[0]
    assert TC.case(e) == (7, 5, 9, 1)
    sd, x, y, state, m = TC.detector_inputs(e, mask)
    want = V.manual_window(sd, x, y, state, m, max_window=e.T)[1]
    worst = max(V.rel_errors(V.manual_window(sd, x, y, state, m, defect=defect, max_window=e.T)[1], want).values())
    print(defect, mask, worst)
    assert worst > 10 * V.GRAD_BOUND


def test_the_defects_left_out_are_defects_the_helpers_know():
    assert set(MASK_DEFECTS) <= set(D.DEFECTS) and MASK_DEFECTS[0] in V.DEFECTS and set(DETECTOR_CANNOT_SHOW) <= set(V.DEFECTS)
    e = TC.DETECTOR[0]                                      # ... and that one indeed cannot show: max_window = T moves nothing
    sd, x, y, state, m = TC.detector_inputs(e, "random")
    a = V.manual_window(sd, x, y, state, m, max_window=e.T)[1]
    b = V.manual_window(sd, x, y, state, m, defect="divisor_max_window", max_window=e.T)[1]
    assert all(np.array_equal(a[k], b[k]) for k in V.KEYS)


# ---- the existing cases have not moved ----------------------------------------------------------------------------------------
# sha256 (first 16 hex digits) over x, y and the mask of the runs None, "random", "zero_row" of every case of D.GRAD_CASES, taken
# before ``case_inputs`` got its output count
TODAY = {(100, 64, 1, 1): "92155e519a6c32f0", (100, 64, 2, 1): "2b7204113e7de1fe", (100, 64, 3, 1): "84a381cf73d1468c",
         (100, 64, 4, 1): "8f7b09c3143620a5", (100, 64, 5, 1): "5f3132537021d8ae", (6, 5, 7, 1): "c771f7648cd593ee",
         (100, 64, 50, 1): "2f16a58ad2eb850c", (128, 256, 9, 1): "871562ec41d427be", (100, 64, 37, 4): "10a83500ebcb2bad",
         (100, 64, 350, 1): "49e378ce3f021cf2"}


@pytest.mark.parametrize("case", D.GRAD_CASES, ids=str)
def test_default_output_count_gives_todays_bits(case):
    h = hashlib.sha256()
    for mask in (None, "random", "zero_row"):
        sd, x, y, m = D.case_inputs(case, mask)
        for a in (x, y) + (() if m is None else (m,)):
            h.update(np.ascontiguousarray(a).tobytes())
        want = R.decoder_state_dict(case[0], case[1], case[3])                  # the precision tests' decoder, regressor included
        assert list(sd) == list(want) and all(np.array_equal(sd[k].numpy(), want[k].numpy()) for k in want)
        assert y.shape == (case[2], 20) and y.dtype == np.float32
    assert h.hexdigest()[:16] == TODAY[case]


def test_an_output_count_redraws_the_regressor_alone():
    case = (6, 5, 7, 1)
    sd, x, y, m = D.case_inputs(case, "random", outputs=3)
    sd0, x0, y0, m0 = D.case_inputs(case, "random")
    assert tuple(sd["regressor.weight"].shape) == (3, 12) and tuple(sd["regressor.bias"].shape) == (3,) and y.shape == (7, 3)
    assert float(sd["regressor.weight"].abs().max()) <= 1.0 / np.sqrt(12.0)                       # nn.Linear's default range
    assert all(np.array_equal(sd[k].numpy(), sd0[k].numpy()) for k in D.KEYS if k.startswith("lstm."))
    assert np.array_equal(x, x0) and m.shape == m0.shape
    again = D.case_inputs(case, "random", outputs=3)[0]
    assert np.array_equal(sd["regressor.weight"].numpy(), again["regressor.weight"].numpy())


# ---- the table contains what it is there for ------------------------------------------------------------------------------------

def _define(header, name):
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(rf"^#define {name} (\d+)\b", f.read(), re.M)
    assert m, (header, name)
    return int(m.group(1))


def test_the_restated_constants_are_the_kernels():
    assert TC.DEC_THREADS == _define("lstm_blocks.h", "DEC_THREADS") and TC.VAD_THREADS == _define("lstm_blocks.h", "VAD_THREADS")
    assert TC.STEP_TILE == _define("dec_train.hip", "DTS_THREADS") == _define("vad_train.hip", "VTS_THREADS")
    assert TC.FRAME_TILE == _define("lstm_blocks.h", "DEC_RROWS") == _define("dec_train.hip", "DTM_FR")
    assert TC.DEC_MAXO == _define("dss_common.h", "DSS_DEC_MAXO")
    assert max(e.H for e in TC.DECODER) <= _define("dss_common.h", "DSS_DEC_MAXH") and max(e.C for e in TC.DECODER) <= _define("dss_common.h", "DSS_DEC_MAXC")
    assert max(e.H for e in TC.DETECTOR) <= _define("dss_common.h", "DSS_VAD_MAXH") and max(e.C for e in TC.DETECTOR) <= _define("dss_common.h", "DSS_VAD_MAXC")


def test_a_detector_window_beyond_the_loss_loops_stride():
    assert any(e.T > TC.VAD_THREADS for e in TC.DETECTOR)


def test_a_detector_window_beyond_the_step_tile_and_within_the_stride():
    assert any(TC.STEP_TILE < e.T <= TC.VAD_THREADS for e in TC.DETECTOR)
    # ... once where a thread's second column is live: a row of max(C, H) + H + 1 columns on 256 threads
    assert any(TC.STEP_TILE < e.T and max(e.C, e.H) + e.H + 1 > TC.STEP_TILE for e in TC.DETECTOR)


def test_a_decoder_trial_beyond_the_loss_bodys_stride():
    assert any(e.T > TC.DEC_THREADS for e in TC.DECODER)


def test_decoder_trials_at_the_frame_tiles_and_at_the_step_tiles_edge():
    lengths = {e.T for e in TC.DECODER}
    assert {TC.FRAME_TILE, 2 * TC.FRAME_TILE, 2 * TC.FRAME_TILE + 1, TC.STEP_TILE, TC.STEP_TILE + 1} <= lengths
    assert {8, 16, 17, 256, 257} <= lengths


@pytest.mark.parametrize("table", (TC.DECODER, TC.DETECTOR), ids=("decoder", "detector"))
def test_hidden_sizes_of_both_odd_residues(table):
    assert {1, 3} <= {e.H % 4 for e in table}
    assert any(e.C % 4 for e in table) and any(e.H == 1 and e.C == 1 for e in table)


def test_one_output_and_the_most_outputs():
    assert {1, TC.DEC_MAXO} <= {e.O for e in TC.DECODER}
    assert all(e.O is None for e in TC.DETECTOR)


def test_masks_and_the_selections():
    for e in TC.DECODER + TC.DETECTOR:
        assert e.masks == ((None, "twos") if e.H == 1 else (None, "random")), e
    assert len(set(TC.DECODER)) == len(TC.DECODER) and len(set(TC.DETECTOR)) == len(TC.DETECTOR)
    assert [TC.ident(e) for e in TC.DECODER_AFTER_STEPS] == ["7-5-9-1-20", "33-17-17-1-20", "6-5-17-1-3"]
    assert [TC.ident(e) for e in TC.DETECTOR_PUBLISH] == ["7-5-9-1", "33-17-17-1"]
    assert TC.RMSPROP_CASES == ((7, 5, 9, 1), (33, 17, 17, 1))
    assert TC.DECODER_REUSE.T == 513 and TC.DETECTOR_REUSE.T == 641 and TC.REUSE_FRAMES == 3
    assert set(TC.DETECTOR_TRIALS) == {(16, 8, 100, 50), (16, 8, 49, 50), (16, 8, 3, 1), (16, 8, 600, 300), (7, 5, 19, 8)}
    assert TC.DECODER_GROUP_FRAMES == (8, 9, 257) == TC.DECODER_GROUP_FRAMES[:2] + (TC.DECODER_GROUP_MAX_FRAMES,)
    assert TC.DETECTOR_GROUP_FRAMES == (16, 17, 300) and TC.DETECTOR_GROUP_WINDOW == 8
    twos = TC.detector_inputs(TC.DETECTOR[3], "twos")[4]
    assert twos.shape == (3, 1) and (twos == 2.0).all() and TC.decoder_inputs(TC.DECODER[4], "twos")[3].shape == (3, 2)
    m = TC.decoder_inputs(TC.DECODER[0], "random")[3]
    assert set(np.unique(m)) == {0.0, 2.0} and TC.decoder_inputs(TC.DECODER[0], None)[3] is None
