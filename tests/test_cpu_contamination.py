"""Host side of the acoustic contamination analysis (Part 12 of include/dss_hip.h, dss_amd/contamination.py) without a GPU:
declarations, every argument check and its reason, the window, the numpy pieces on hand-built inputs, and the float64 statement
of the method (tests/contamination_reference.py) held to scipy and to a planted leak."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import contamination_cases as cases
import contamination_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dss_contam_check_params", "dss_contam_check_window", "dss_contam_frames_for", "dss_contam_check_call", "dss_contam_result_size",
       "dss_contam_create", "dss_contam_destroy", "dss_contam_moments", "dss_contam_moments_dev", "dss_contam_plan")
# the planted case (contamination_reference.planted_case, seed 11), artifact detection on: recorded from the reference
PLANT_P, PLANT_MEASURE, CLEAN_P, CLEAN_MEASURE = 0.0, 0.5562, 0.7143, 0.0988


def test_entry_points_are_declared_and_exported():
    from dss_amd import _lib, contamination
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dss_hip.h")).read(), flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name
    for name in ("hamming_symmetric", "ContaminationGPU", "contamination_matrix", "statistical_criterion", "detect_artifacts",
                 "frame_mask", "speech_periods", "contamination_analysis", "kept_bins"):
        assert hasattr(contamination, name), name
    assert C.sizeof(contamination.ContamParams) == 24                                # the header's six ints


def test_every_refusal_and_its_reason():
    from dss_amd import _lib, contamination
    L = _lib.load()
    P = contamination.ContamParams
    good = dict(nperseg=200, hop=20, bin_lo=14, n_bins=21, max_lag=25, reserved=0)
    assert L.dss_contam_check_params(C.addressof(P(**good))) == 0
    for change in (dict(nperseg=2, bin_lo=0, n_bins=2, hop=1), dict(n_bins=31), dict(n_bins=1), dict(max_lag=0), dict(max_lag=4096),
                   dict(bin_lo=80), dict(hop=100), dict(nperseg=16, hop=4, bin_lo=2, n_bins=4, max_lag=3),
                   dict(nperseg=1024, hop=32, bin_lo=100)):
        assert L.dss_contam_check_params(C.addressof(P(**{**good, **change}))) == 0, change
    for change, message in ((dict(nperseg=1), b"nperseg must be at least 2"), (dict(nperseg=2049), b"nperseg up to 2048"),
                            (dict(hop=0), b"hop between frames must be at least 1"), (dict(n_bins=0), b"keeps 0 bins; 1 to 31"),
                            (dict(n_bins=32), b"keeps 32 bins; 1 to 31"), (dict(bin_lo=-1), b"bins -1 .. 19 lie outside the 101 bins"),
                            (dict(bin_lo=81), b"bins 81 .. 101 lie outside the 101 bins of a 200-row window"),
                            (dict(max_lag=-1), b"maximum lag of 0 to 4096"), (dict(max_lag=4097), b"maximum lag of 0 to 4096"),
                            (dict(nperseg=2048, hop=2048), b"do not fit the kernel's 81920 bytes of LDS")):
        assert L.dss_contam_check_params(C.addressof(P(**{**good, **change}))) == -1 and message in L.dss_last_error(), change
    assert L.dss_contam_check_params(None) == -1 and b"no parameters" in L.dss_last_error()

    for n in range(200, 3000, 7):
        assert L.dss_contam_frames_for(n, 200, 20, 25) == (n - 200) // 20 + 1
    assert contamination.frames_for(2600, 200, 20, 25) == 121
    assert contamination.frames_for(600, 200, 20, 25) == 21                           # fewer frames than lags is allowed

    def refused(message, *args):
        with pytest.raises(_lib.DssError, match=message):
            contamination.frames_for(*args)
    refused("199 rows is shorter than one window \\(200 rows\\)", 199, 200, 20, 25)
    refused("nperseg must be at least 2", 100, 1, 1, 0)
    refused("hop between frames must be at least 1", 1000, 200, 0, 25)
    refused("negative maximum lag", 1000, 200, 20, -1)
    refused("exceed the 32-bit frame index", 2**40, 4, 1, 25)
    assert L.dss_contam_frames_for(2**31 - 1 - 50 - 64 + 3, 4, 1, 25) == 2**31 - 1 - 50 - 64      # the largest allowed
    assert L.dss_contam_frames_for(2**31 - 1 - 50 - 64 + 4, 4, 1, 25) == -1

    off = (C.c_longlong * 7)()
    p = P(**good)
    assert L.dss_contam_result_size(C.addressof(p), 3, C.addressof(off)) == 51 + 21 + 2 * 51 * 21 + 2 * 51 * 3 * 21 + 51 * 3 * 441
    assert list(off) == [0, 51, 72, 72 + 1071, 72 + 2142, 72 + 2142 + 3213, 72 + 2142 + 6426]
    assert L.dss_contam_result_size(C.addressof(p), 0, None) == -1 and b"0 channels" in L.dss_last_error()
    assert L.dss_contam_result_size(C.addressof(P(**{**good, "n_bins": 40})), 3, None) == -1 and b"keeps 40 bins" in L.dss_last_error()
    assert L.dss_contam_result_size(C.addressof(p), 65535, None) == 51 + 21 + 2 * 51 * 21 + 65535 * 51 * (2 * 21 + 441)
    assert L.dss_contam_result_size(C.addressof(p), 65536, None) == -1
    assert b"65536 channels are too many for one launch (up to 65535)" in L.dss_last_error()

    # the sizes of a call, as both forms check them before they touch a device
    assert L.dss_contam_check_call(C.addressof(p), 2600, 19, 17) == 121
    assert L.dss_contam_check_call(C.addressof(p), 2600, 3, 3) == 121
    for args, message in (((2600, 3, 0), b"0 channels in rows of 3 values"), ((2600, 3, -1), b"-1 channels in rows of 3 values"),
                          ((2600, 2, 3), b"3 channels in rows of 2 values"),
                          ((2600, 70000, 65536), b"65536 channels are too many for one launch (up to 65535)"),
                          ((199, 3, 3), b"199 rows is shorter than one window (200 rows)")):
        assert L.dss_contam_check_call(C.addressof(p), *args) == -1 and message in L.dss_last_error(), args
    assert L.dss_contam_check_call(C.addressof(P(**{**good, "hop": 0})), 2600, 3, 3) == -1 and b"hop between frames" in L.dss_last_error()
    assert L.dss_contam_check_call(None, 2600, 3, 3) == -1 and b"no parameters" in L.dss_last_error()
    assert L.dss_contam_check_call(C.addressof(P(**{**good, "nperseg": 4, "hop": 1, "bin_lo": 0, "n_bins": 2})), 2**40, 3, 3) == -1
    assert b"exceed the 32-bit frame index" in L.dss_last_error()

    # the window is data of the caller and is checked before a device is asked for: create fails with the window's reason
    w = np.ones(200)
    assert L.dss_contam_check_window(C.addressof(p), w.ctypes.data) == 0
    assert L.dss_contam_check_window(C.addressof(P(**{**good, "hop": 0})), w.ctypes.data) == -1 and b"hop between frames" in L.dss_last_error()
    assert L.dss_contam_create(C.addressof(P(**{**good, "hop": 0})), w.ctypes.data) is None and b"hop between frames" in L.dss_last_error()
    for bad, message in ((None, b"missing window"), (np.zeros(200), b"the window is all zero"),
                         (np.where(np.arange(200) == 199, np.nan, 1.0), b"the window holds a non-finite value"),
                         (np.where(np.arange(200) == 0, np.inf, 1.0), b"the window holds a non-finite value"),
                         (np.where(np.arange(200) == 7, -np.inf, 0.0), b"the window holds a non-finite value")):
        ptr = None if bad is None else bad.ctypes.data
        assert L.dss_contam_check_window(C.addressof(p), ptr) == -1 and message in L.dss_last_error(), message
        assert L.dss_contam_create(C.addressof(p), ptr) is None and message in L.dss_last_error(), message
    one = np.where(np.arange(200) == 199, -1e-300, 0.0)                                # its square underflows: still all zero
    assert L.dss_contam_check_window(C.addressof(p), one.ctypes.data) == -1 and b"all zero" in L.dss_last_error()
    one[199] = 1e-150
    assert L.dss_contam_check_window(C.addressof(p), one.ctypes.data) == 0
    # the handle forms refuse a missing handle instead of faulting
    assert L.dss_contam_moments(None, None, 1000, 3, 3, None, None, None) == -1 and b"bad arguments" in L.dss_last_error()
    assert L.dss_contam_moments_dev(None, None, 1000, 3, 3, None, None, None, None) == -1
    L.dss_contam_destroy(None)
    # the Python class refuses before it needs a device
    with pytest.raises(_lib.DssError, match="keeps 0 bins"):
        contamination.ContaminationGPU(1000, band=(71, 74))
    with pytest.raises(_lib.DssError, match="keeps 41 bins"):
        contamination.ContaminationGPU(1000, band=(70, 270))
    with pytest.raises(_lib.DssError, match="hop between frames"):
        contamination.ContaminationGPU(10, window=1.0, spg_fs=50)


def test_kept_bins_follow_the_definition_at_a_band_edge_on_a_bin():
    from dss_amd.contamination import kept_bins
    assert list(kept_bins(1000, 200, (70, 170))) == list(range(14, 35))
    assert list(kept_bins(1000, 200, (70.001, 169.999))) == list(range(15, 34))
    assert list(kept_bins(1000, 16, (125, 312.5))) == [2, 3, 4, 5]
    assert len(kept_bins(1000, 200, (71, 74))) == 0
    # fs 1002, 200 rows: bins 14 and 34 lie at 14 * 1002 / 200 = 70.14 and 170.34 exactly as the definition computes them; taken
    # as k / (200 / 1002) they come out one unit in the last place higher, and the upper edge would lose its bin
    assert 14 * 1002 / 200 == 70.14 and 34 * 1002 / 200 == 170.34 and np.fft.rfftfreq(200, 1 / 1002)[34] > 170.34
    for fs, nperseg, band in ((1002, 200, (70.14, 170.34)), (501, 100, (5.01, 50.1)), (1017.25, 203, (70, 170)), (30000, 6000, (70, 170))):
        got = kept_bins(fs, nperseg, band)
        assert np.array_equal(got, ref.kept_bins(fs, nperseg, band)), fs
    assert list(kept_bins(1002, 200, (70.14, 170.34))) == list(range(14, 35))
    assert list(kept_bins(501, 100, (5.01, 50.1))) == list(range(1, 11))


def test_window_and_spectrogram_against_scipy():
    from scipy.signal import get_window, spectrogram
    from dss_amd.contamination import hamming_symmetric
    for n in (2, 3, 16, 199, 200, 400):
        assert np.array_equal(hamming_symmetric(n), get_window("hamming", n, fftbins=False)), n
        assert np.allclose(ref.hamming(n), hamming_symmetric(n), rtol=0, atol=16 * ref.U)       # the cosine of an argument rounded near 2 pi
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2600, 2))
    w = hamming_symmetric(200)
    bins = ref.kept_bins(1000, 200, (70, 170))
    assert list(bins) == list(range(14, 35))
    got, absseg = ref.spectrogram(x, w, 200, 20, bins)
    assert got.shape == (121, 2, 21) and absseg.shape == (121, 2)
    for c in range(2):
        f, _, want = spectrogram(x[:, c], fs=1000, window=w, nperseg=200, noverlap=180, nfft=200, detrend=False, mode="magnitude")
        assert np.array_equal(f[bins], bins * 5.0)
        scale = np.sqrt(1.0 / (1000 * (w * w).sum()))                                 # scipy's constant factor (scaling='density')
        assert np.allclose(got[:, c].T * scale, want[bins], rtol=0, atol=1e-12 * np.max(want))


def test_frame_mask_speech_periods_and_artifacts_on_hand_built_inputs():
    from dss_amd.contamination import detect_artifacts, frame_mask, periods_mask, speech_periods
    keep = np.ones(30, dtype=bool)
    keep[13] = False
    # frames of 8 rows every 4: frame t covers rows 4 t .. 4 t + 7; row 13 lies in frames 2 and 3; row 28.. belong to no frame
    assert list(frame_mask(keep, 8, 4)) == [True, True, False, False, True, True]
    assert list(ref.frame_mask(keep, 8, 4)) == [True, True, False, False, True, True]
    keep[29] = False
    assert list(frame_mask(keep, 8, 4)) == [True, True, False, False, True, True]
    keep[0] = False
    assert list(frame_mask(keep, 8, 4)) == [False, True, False, False, True, True]
    assert frame_mask(np.ones(5, dtype=bool), 8, 4).shape == (0,)

    labels = np.array([0, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1])
    p = speech_periods(labels)
    assert p.dtype == np.float32 and p.shape == (2, 2)                                # the unpaired last change is dropped
    assert np.array_equal(p, np.array([[2, 4], [7, 7]], dtype=np.float32) * np.float32(0.01))
    assert speech_periods(np.zeros(10, dtype=int)).shape == (0, 2)
    m = periods_mask(p, 100, 1000)                                                    # usable as select_periods
    assert list(np.where(m)[0]) == list(range(20, 41)) + [70]

    # ten channels of +1, -1, +1, ...: less the 3-sample moving average d = +-2/3 inside (+-1 at the two ends, where the window
    # holds two samples), median 0, median |d| = 2/3: at factor 1.6 the threshold is 1.0667 and nothing crosses
    T = 400
    x = np.tile(np.where(np.arange(T) % 2 == 0, 1.0, -1.0)[:, None], (1, 10))
    assert not detect_artifacts(x, 100, span=0.03, factor=1.6, ratio=0.1, safety=0.05).any()
    x[200, 3] += 50                                                                   # the spike also moves the averages of rows 199 and 201
    art = detect_artifacts(x, 100, span=0.03, factor=1.6, ratio=0.1, safety=0.05)      # one channel of ten is enough at ratio 0.1
    assert list(np.where(art)[0]) == list(range(194, 207))
    assert not detect_artifacts(x, 100, span=0.03, factor=1.6, ratio=0.2, safety=0.05).any()   # two are needed
    x[200, 7] += 50
    assert list(np.where(detect_artifacts(x, 100, span=0.03, factor=1.6, ratio=0.2, safety=0.0))[0]) == [199, 200, 201]
    x[1, :] += 50                                                                     # at the start: the widening stops at row 0
    assert list(np.where(detect_artifacts(x, 100, span=0.03, factor=1.6, ratio=0.5, safety=0.03))[0]) == [0, 1, 2, 3, 4, 5]


def test_criterion_on_hand_built_matrices():
    from dss_amd.contamination import contamination_matrix, statistical_criterion
    B = 10
    M = np.full((B, B), 0.1) + 0.5 * np.eye(B)
    sur, measure, p = statistical_criterion(M, 2000, seed=3)
    assert sur.dtype == np.float32 and sur.shape == (2000,)
    assert measure == pytest.approx(0.6) and p == 0.0                                  # one permutation in 3628800 is the identity
    assert np.all(sur <= np.float32(0.6))
    sur, measure, p = statistical_criterion(np.full((B, B), 0.25), 500)
    assert p == 1.0 and measure == 0.25 and np.all(sur == np.float32(0.25))
    a, b = statistical_criterion(M, 300, seed=5), statistical_criterion(M, 300, seed=5)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[0], statistical_criterion(M, 300, seed=6)[0])
    rs, rm, rp = ref.criterion(M, 300, seed=5)
    assert np.array_equal(a[0], rs.astype(np.float32)) and a[1] == pytest.approx(rm) and a[2] == rp
    # the first permutation is the generator's
    perm = np.random.Generator(np.random.PCG64(5)).permutation(B)
    assert a[0][0] == np.float32(np.mean(M[np.arange(B), perm]))
    # a NaN on the diagonal (a bin constant in every channel): nothing to compare, so no verdict -- not P = 0
    hole = M.copy()
    hole[:, 4] = np.nan
    for fn in (statistical_criterion, ref.criterion):
        sur, measure, p = fn(hole, 50, seed=1)
        assert np.isnan(measure) and np.isnan(p) and len(sur) == 50, fn
    r0 = np.array([[[0.1, np.nan], [np.nan, 0.3]], [[0.2, np.nan], [np.nan, -0.5]]])
    got = contamination_matrix(r0)
    assert got[0, 0] == 0.2 and got[1, 1] == 0.3 and np.isnan(got[0, 1]) and np.isnan(got[1, 0])
    assert np.array_equal(got, ref.contamination_matrix(r0), equal_nan=True)


def test_correlations_from_moments_equal_the_two_pass_reference():
    from dss_amd.contamination import Moments, correlations_from_moments
    rng = np.random.default_rng(2)
    brain, audio = rng.standard_normal((700, 3)), rng.standard_normal(700)
    brain[:, 1] = 2.5                                                                 # a constant channel: NaN
    keep = np.ones(700, dtype=bool)
    keep[300:310] = False
    day = ref.Day(brain, audio, 1000, max_lag=0.1, keep=keep)
    r = day.correlations()
    m, d = day.moments(day.A[day.fm].mean(axis=0))
    got = correlations_from_moments(Moments(m["n"], None, m["sa"], m["saa"], m["sb"], m["sbb"], m["sab"]))
    assert np.array_equal(np.isnan(got), np.isnan(r)) and np.all(np.isnan(r[:, 1])) and not np.isnan(r[:, 0]).any()
    ok = ~np.isnan(r)
    assert np.all(np.abs(got - r)[ok] <= ref.r_bound(m, d)[ok])


@pytest.fixture(scope="module")
def planted():
    out = {}
    for plant in (True, False):
        from dss_amd.contamination import detect_artifacts
        brain, audio = ref.planted_case(plant)
        day = ref.Day(brain, audio, ref.PLANT_FS, keep=~detect_artifacts(brain, ref.PLANT_FS))
        r = day.correlations()
        out[plant] = (day, r, ref.criterion(ref.contamination_matrix(r[day.L])))
    return out


def test_planted_leak_is_found_and_its_absence_is_not(planted):
    day, r, (sur, measure, p) = planted[True]
    assert day.W == 991 and r.shape == (51, ref.PLANT_C, 21, 21)
    rc = r[:, ref.PLANT_CHANNEL]
    lag, i, j = np.unravel_index(np.nanargmax(rc), rc.shape)
    assert lag == day.L and i == j                                                    # the peak: lag 0, on the diagonal
    print(f"planted: measure {measure:.4f}, P {p:.4f}; clean: measure {planted[False][2][1]:.4f}, P {planted[False][2][2]:.4f}")
    assert p < 0.05 and p == PLANT_P and measure == pytest.approx(PLANT_MEASURE, abs=5e-5)
    _, _, (_, measure, p) = planted[False]
    assert p > 0.05 and p == pytest.approx(CLEAN_P, abs=5e-5) and measure == pytest.approx(CLEAN_MEASURE, abs=5e-5)


def _plan(L, p, n_rows, n_channels):
    plan = (C.c_int * 6)()
    rc = L.dss_contam_plan(C.addressof(p), n_rows, n_channels, C.addressof(plan))
    return rc, tuple(plan)


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_reaches_the_plan_it_is_there_for_and_the_reference_agrees_with_itself(name):
    """The case table of tests/contamination_cases.py without a GPU: the operator gives the shape the table states, the library
    plans the launch the case is there to reach, and the reference alone -- its one-pass sums through correlations_from_moments
    against its two-pass correlations -- meets every condition the GPU test holds the kernels to."""
    from dss_amd import contamination
    from dss_amd.contamination import Moments, correlations_from_moments
    s = cases.spec(name)
    op, brain, audio, keep = cases.build(name)
    day = cases.day(name)
    assert cases.shape_of(day) == s.shape
    nperseg, hop, bin_lo, B, lag, W = s.shape
    assert (int(round(op.get("window", 0.2) * op["fs"])), int(round(op["fs"] / op.get("spg_fs", 50)))) == (nperseg, hop)
    inside = contamination.kept_bins(op["fs"], nperseg, op.get("band", (70, 170)))
    assert (int(inside[0]), len(inside)) == (bin_lo, B) and contamination.frames_for(s.T, nperseg, hop, lag) == W
    p = contamination.ContamParams(nperseg, hop, bin_lo, B, lag, 0)
    assert contamination.launch_plan(p, s.T, s.C) == s.plan
    frames, tiles, chunks, per, Z, lgn = s.plan
    if name in ("many_tiles", "default_long", "planted", "one_chunk"):
        assert per > 1 and (chunks == 1 or tiles % per)                               # several tiles per chunk, a shorter last chunk
    else:
        assert per == 1
    if name == "odd_window":
        assert nperseg % 2 == 1 and bin_lo + B - 1 == nperseg // 2
    if name == "apart":
        assert hop > ((nperseg + 3) & ~3) and np.isnan(brain).any() and np.isnan(audio).any()
    if name == "abutting":
        assert hop == nperseg < ((nperseg + 3) & ~3)
    if name == "one_chunk":
        assert brain.strides == (523 * 8, 8)
    if name == "lds_edge":
        assert 1800 < nperseg < 1900 and cases.params_accepted(nperseg, 1, bin_lo, B, 0)
        assert not cases.params_accepted(nperseg + 1, 1, bin_lo, B, 0)
        assert b"do not fit the kernel's 81920 bytes of LDS" in _lib_error()

    want, bound = day.moments(cases.kept_mean(day))
    r_want = day.correlations()
    assert np.isfinite(r_want[~np.isnan(r_want)]).all() and all(np.isfinite(want[k]).all() for k in want)
    r = correlations_from_moments(Moments(want["n"], None, want["sa"], want["saa"], want["sb"], want["sbb"], want["sab"]))
    assert np.array_equal(np.isnan(r), np.isnan(r_want))
    ok = ~np.isnan(r_want)
    rb = ref.r_bound(want, bound)
    assert ok.any() == (name not in cases.NO_CORRELATION)
    if ok.any():
        print(f"{name}: reference against itself, max |difference| / bound {np.max(np.abs(r - r_want)[ok] / rb[ok]):.3g}, "
              f"median bound {np.median(rb[ok]):.3g}")
        assert np.all(np.abs(r - r_want)[ok] <= rb[ok]) and np.median(rb[ok]) < 1e-9
    cases.check_exact(name, want["n"], cases.kept_mean(day), want, r_want)
    cases.check_exact(name, want["n"], cases.kept_mean(day), want, r)


def _lib_error():
    from dss_amd import _lib
    return _lib.load().dss_last_error()


def test_plan_refuses_what_the_calls_refuse_and_every_plan_covers_its_frames_and_lags():
    from dss_amd import _lib, contamination
    L = _lib.load()
    P = contamination.ContamParams
    good = dict(nperseg=200, hop=20, bin_lo=14, n_bins=21, max_lag=25, reserved=0)
    p = P(**good)
    assert _plan(L, p, 2600, 3) == (0, (121, 4, 4, 1, 2, 7))
    assert contamination.launch_plan(p, 2600, 3)._fields == ("frames", "tiles", "chunks", "tiles_per_chunk", "lag_groups", "lags_per_wave")
    for args in ((2600, 0), (2600, -1), (2600, 65536), (199, 3), (2**40, 3)):
        assert L.dss_contam_check_call(C.addressof(p), args[0], args[1], args[1]) == -1
        reason = L.dss_last_error()
        assert L.dss_contam_plan(C.addressof(p), *args, C.addressof((C.c_int * 6)())) == -1 and L.dss_last_error() == reason, args
        assert len(reason) > 10
    for change in (dict(hop=0), dict(n_bins=32), dict(nperseg=2048, hop=2048), dict(max_lag=4097)):
        bad = P(**{**good, **change})
        assert L.dss_contam_check_call(C.addressof(bad), 2600, 3, 3) == -1
        reason = L.dss_last_error()
        assert _plan(L, bad, 2600, 3)[0] == -1 and L.dss_last_error() == reason, change
    assert L.dss_contam_plan(None, 2600, 3, C.addressof((C.c_int * 6)())) == -1 and b"no parameters" in L.dss_last_error()
    assert L.dss_contam_plan(C.addressof(p), 2600, 3, None) == -1 and b"nowhere to write the plan" in L.dss_last_error()
    with pytest.raises(_lib.DssError, match="199 rows is shorter than one window"):
        contamination.launch_plan(p, 199, 3)

    # every chunk holds a tile, the chunks cover the tiles and the waves cover the lags, over a sweep of (W, C, L)
    seen = set()
    for lag in (0, 1, 3, 15, 16, 17, 25, 31, 32, 47, 48, 63, 64, 100, 1000, 4096):
        q = P(nperseg=16, hop=4, bin_lo=2, n_bins=4, max_lag=lag, reserved=0)
        for W in (1, 2, 31, 32, 33, 64, 65, 95, 96, 97, 991, 1014, 1925, 5000, 16385, 100001):
            for Cn in (1, 2, 3, 9, 12, 40, 127, 128, 129, 255, 256, 257, 511, 512, 513, 520, 65535):
                rc, (frames, tiles, chunks, per, Z, lgn) = _plan(L, q, 16 + 4 * (W - 1) + 3, Cn)
                assert rc == 0 and frames == W and tiles == (W + 31) // 32, (lag, W, Cn)
                assert chunks >= 1 and per >= 1 and chunks * per >= tiles > (chunks - 1) * per, (lag, W, Cn)
                assert 1 <= lgn <= 8 and Z * 4 * lgn >= 2 * lag + 1 > (Z - 1) * 4 * 8, (lag, W, Cn)
                assert chunks == 1 or (chunks - 1) * Cn * Z < 512 + Cn * Z, (lag, W, Cn)             # about 512 workgroups
                seen.add((chunks == 1, per == 1, tiles % per == 0))
    # (one chunk, one tile per chunk, a full last chunk): the sweep reaches every combination there is -- one chunk and chunks of
    # one tile are always full
    assert seen == {(True, True, True), (True, False, True), (False, True, True), (False, False, True), (False, False, False)}
