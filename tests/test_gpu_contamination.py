"""The correlation kernels of the acoustic contamination analysis (csrc/contamination.hip, Part 12 of include/dss_hip.h) on the
GPU against the float64 statement of the method (tests/contamination_reference.py).  Every sum and every finite correlation is
compared within the bound that module derives (the DFT's n-term sums, propagated through the P-term sums into r to first order);
each case prints max |difference| / bound.  The shapes are the smallest that reach every path: 121 frames at the default operator
(three full tiles of 32 and a partial one; 51 lags in two lag groups of the grid, whose waves hold 7, 7, 7, 7 and 7, 7, 7, 2 lags), 3 and 17
channels, frames masked inside, at a tile edge and at both ends; a small operator whose lags cross tile edges and leave waves
with fewer lags than their share, or none; fewer frames than lags; a constant channel."""
import numpy as np
import pytest

import contamination_reference as ref

pytestmark = pytest.mark.gpu

NAMES = ("n", "sa", "saa", "sb", "sbb", "sab")


def _keep_default():
    """Per-sample mask at fs 1000 (frames of 200 rows every 20): drops frames 0, 31 .. 40 (across a tile edge), 61 .. 70 and 120."""
    keep = np.ones(2600, dtype=bool)
    keep[0] = False                      # only frame 0 holds row 0
    keep[819] = False                    # frames 31 .. 40 hold row 819 (31 * 20 + 199)
    keep[1400] = False                   # frames 61 .. 70
    keep[2599] = False                   # only frame 120
    return keep


def _case(name):
    rng = np.random.default_rng(4)
    wide = rng.standard_normal((2600, 19)) * rng.uniform(0.5, 20.0, size=19) + rng.uniform(-3, 3, size=19)
    audio = 50.0 * rng.standard_normal(2600)
    wide[:, 2] += 0.05 * audio
    op = dict(fs=1000)
    if name == "default_c3":
        return op, wide[:, :3], audio, None
    if name == "default_c3_mask":
        return op, wide[:, :3], audio, _keep_default()
    if name == "default_c17_mask":
        return op, wide[:, 1:18], audio, _keep_default()
    if name == "small_operator":         # nperseg 16, hop 4, bins 2 .. 5, L 3, 40 frames
        keep = np.ones(172, dtype=bool)
        keep[100] = False
        return dict(fs=1000, window=0.016, spg_fs=250, band=(125, 312.5), max_lag=0.012), wide[:172, :5], audio[:172], keep
    if name == "fewer_frames_than_lags":  # 21 frames, L 25
        return op, wide[:600, :2], audio[:600], None
    if name == "constant_channel":
        x = wide[:2600, :3].copy()
        x[:, 1] = -7.25
        return op, x, audio, None
    raise KeyError(name)


CASES = ("default_c3", "default_c3_mask", "default_c17_mask", "small_operator", "fewer_frames_than_lags", "constant_channel")


@pytest.fixture(scope="module")
def results():
    """Every case once: the library's sums from host buffers, and the reference's spectrograms.  Shared, never written."""
    from dss_amd.contamination import ContaminationGPU
    out = {}
    for name in CASES:
        op, brain, audio, keep = _case(name)
        g = ContaminationGPU(**op)
        m = g.moments(brain, audio, keep)
        shape = (g.nperseg, g.hop, g.bin_lo, g.n_bins, g.max_lag, g.frames(len(brain)))
        g.close()
        for v in m:
            v.setflags(write=False)
        out[name] = (m, ref.Day(brain, audio, keep=keep, **op), shape)
    return out


@pytest.mark.parametrize("name", CASES)
def test_sums_and_correlations_within_the_derived_bounds(results, name):
    from dss_amd.contamination import correlations_from_moments
    m, day, shape = results[name]
    assert shape == (day.nperseg, day.hop, int(day.bins[0]), len(day.bins), day.L, day.W)
    if name.startswith("default"):
        assert shape == (200, 20, 14, 21, 25, 121)
    if name == "small_operator":
        assert shape == (16, 4, 2, 4, 3, 40)
    # the shift is the mean of the kept audio frames, to rounding; the reference takes the library's value as it is
    assert np.allclose(m.shift, day.A[day.fm].mean(axis=0), rtol=1e-12, atol=0)
    want, bound = day.moments(m.shift)
    assert np.array_equal(m.n, want["n"])
    for key in NAMES[1:]:
        got = getattr(m, key)
        assert got.shape == want[key].shape, key
        live = bound[key] > 0
        print(f"{name} {key}: max |difference| / bound {np.max(np.abs(got - want[key])[live] / bound[key][live]):.3g}")
        assert np.all(np.abs(got - want[key]) <= bound[key]), key
    r, r_want = correlations_from_moments(m), day.correlations()
    assert r.shape == r_want.shape == (2 * day.L + 1, day.N.shape[1], len(day.bins), len(day.bins))
    assert np.array_equal(np.isnan(r), np.isnan(r_want))                               # nothing skipped that the reference defines
    ok = ~np.isnan(r_want)
    rb = ref.r_bound(want, bound)
    print(f"{name} r: max |difference| / bound {np.max(np.abs(r - r_want)[ok] / rb[ok]):.3g}, largest bound {np.max(rb[ok]):.3g}")
    assert np.all(np.abs(r - r_want)[ok] <= rb[ok]) and np.median(rb[ok]) < 1e-9             # and the bound says something


def test_masked_frames_empty_lags_and_a_constant_channel(results):
    from dss_amd.contamination import contamination_matrix, correlations_from_moments
    m, day, _ = results["default_c3_mask"]
    assert int(day.fm.sum()) == 121 - 1 - 10 - 10 - 1 and m.n[25] == day.fm.sum() and m.n[0] < m.n[25]
    assert not np.array_equal(m.n, results["default_c3"][0].n)
    m, day, _ = results["fewer_frames_than_lags"]
    assert day.W == 21
    assert list(m.n) == [max(0, 21 - abs(l)) for l in range(-25, 26)]
    r = correlations_from_moments(m)
    for li in (0, 1, 2, 3, 4, 46, 47, 48, 49, 50):                                    # |lag| >= 21: no frames
        assert m.n[li] == 0 and not m.sab[li].any() and not m.sb[li].any() and not m.sa[li].any() and np.all(np.isnan(r[li]))
    assert np.all(np.isnan(r[5])) and m.n[5] == 1                                     # one pair is no correlation either
    assert not np.isnan(r[6:45]).any()
    m, day, _ = results["constant_channel"]
    r = correlations_from_moments(m)
    assert np.all(np.isnan(r[:, 1])) and not np.isnan(r[:, 0]).any() and not np.isnan(r[:, 2]).any()
    M = contamination_matrix(r[25])
    assert not np.isnan(M).any() and np.array_equal(M, np.maximum(r[25, 0], r[25, 2]))   # nanmax skips the constant channel


def test_host_device_and_repeated_calls_agree_bit_for_bit_and_strided_rows_are_read_in_place(results):
    import torch
    from dss_amd.contamination import ContaminationGPU
    _, brain, audio, keep = _case("default_c17_mask")                                 # columns 1 .. 17 of rows of 19: a strided view
    assert brain.strides == (19 * 8, 8)
    m = results["default_c17_mask"][0]
    g = ContaminationGPU(1000)
    again = g.moments(brain, audio, keep)
    wide = torch.from_numpy(np.ascontiguousarray(brain.base if brain.base is not None else brain)).cuda()
    view = wide[:, 1:18]
    assert view.stride() == (19, 1) and view.data_ptr() == wide.data_ptr() + 8
    dev = g.moments_torch(view, torch.from_numpy(audio).cuda(), keep)
    packed = g.moments(np.ascontiguousarray(brain), audio, keep)
    one = g.moments(brain[:, 4], audio, keep)                                         # one channel given as a vector
    g.close()
    for k, key in enumerate(m._fields):
        assert np.array_equal(getattr(again, key), getattr(m, key)), key
        assert np.array_equal(dev[k].cpu().numpy(), getattr(m, key)), key
        assert np.array_equal(getattr(packed, key), getattr(m, key)), key
    assert np.array_equal(one.sab[:, 0], m.sab[:, 4]) and np.array_equal(one.sbb[:, 0], m.sbb[:, 4])   # a channel's bits do not depend on the others


def test_a_live_handle_refuses_bad_calls_with_their_reasons(results):
    """The refusals that need a handle (the C ABI's) or an operator (Python's): each before any launch, each with its reason, and
    the handle works afterwards."""
    import ctypes as C
    import torch
    from dss_amd import _lib
    from dss_amd.contamination import ContaminationGPU
    _, brain, audio, _ = _case("default_c3")
    brain = np.ascontiguousarray(brain)
    g = ContaminationGPU(1000)
    L, h = g._L, g._h
    out = np.empty(g._layout(3)[7])
    b, a, o = brain.ctypes.data, audio.ctypes.data, out.ctypes.data
    d_brain, d_audio = torch.from_numpy(brain).cuda(), torch.from_numpy(audio).cuda()
    d_out = torch.empty(len(out), dtype=torch.float64, device="cuda")
    db, da, do = d_brain.data_ptr(), d_audio.data_ptr(), d_out.data_ptr()
    for args in ((None, a, o), (b, None, o), (b, a, None)):                           # a missing buffer, the handle being there
        assert L.dss_contam_moments(h, args[0], 2600, 3, 3, args[1], None, args[2]) == -1 and b"bad arguments" in L.dss_last_error()
    for args in ((None, da, do), (db, None, do), (db, da, None)):
        assert L.dss_contam_moments_dev(h, args[0], 2600, 3, 3, args[1], None, args[2], None) == -1
        assert b"bad arguments" in L.dss_last_error()
    for sizes, message in (((2600, 2, 3), b"3 channels in rows of 2 values"), ((2600, 3, 0), b"0 channels in rows of 3 values"),
                           ((2600, 70000, 65536), b"65536 channels are too many for one launch (up to 65535)"),
                           ((199, 3, 3), b"199 rows is shorter than one window (200 rows)")):
        assert L.dss_contam_moments(h, b, *sizes, a, None, o) == -1 and message in L.dss_last_error(), sizes
        assert L.dss_contam_moments_dev(h, db, *sizes, da, None, do, None) == -1 and message in L.dss_last_error(), sizes

    with pytest.raises(ValueError, match="audio holds 2599 samples, the brain signals 2600 rows"):
        g.moments(brain, audio[:-1])
    with pytest.raises(ValueError, match="audio holds 2599 samples, the brain signals 2600 rows"):
        g.moments_torch(d_brain, d_audio[:-1])
    with pytest.raises(ValueError, match=r"keep must hold one value per sample \(2600\), not 2599"):
        g.moments(brain, audio, np.ones(2599, dtype=bool))
    with pytest.raises(ValueError, match=r"keep must hold one value per sample \(2600\), not 2601"):
        g.moments_torch(d_brain, d_audio, np.ones(2601, dtype=bool))
    with pytest.raises(ValueError, match="audio must be a CUDA float64 tensor"):
        g.moments_torch(d_brain, torch.from_numpy(audio))                              # a host tensor
    with pytest.raises(ValueError, match="audio must be a CUDA float64 tensor"):
        g.moments_torch(d_brain, d_audio.float())                                      # float32
    with pytest.raises(_lib.DssError, match="199 rows is shorter than one window"):
        g.moments(brain[:199], audio[:199])
    with pytest.raises(_lib.DssError, match="199 rows is shorter than one window"):
        g.moments_torch(d_brain[:199], d_audio[:199])
    assert g.frames(2600) == 121 and list(g.lags) == list(range(-25, 26))
    assert np.array_equal(g.frequencies, ref.kept_bins(1000, 200, (70, 170)) * 5.0)

    m = g.moments(brain, audio)                                                        # and the handle is none the worse for it
    g.close()
    for key in m._fields:
        assert np.array_equal(getattr(m, key), getattr(results["default_c3"][0], key)), key


def test_planted_leak_end_to_end():
    """contamination_analysis on the planted case of tests/test_cpu_contamination.py: the same verdicts, and the reference's values."""
    from dss_amd.contamination import contamination_analysis, detect_artifacts
    import test_cpu_contamination as cpu
    for plant, p_want, measure_want in ((True, cpu.PLANT_P, cpu.PLANT_MEASURE), (False, cpu.CLEAN_P, cpu.CLEAN_MEASURE)):
        brain, audio = ref.planted_case(plant)
        res = contamination_analysis(brain, audio, ref.PLANT_FS)
        assert res.surrogate_measures.shape == (10000,) and res.surrogate_measures.dtype == np.float32
        assert res.matrix.shape == (21, 21) and res.correlations.shape == (51, ref.PLANT_C, 21, 21)
        print(f"plant {plant}: measure {res.dataset_measure:.4f}, P {res.criterion_value:.4f}")
        assert (res.criterion_value < 0.05) == plant
        assert res.criterion_value == pytest.approx(p_want, abs=5e-5) and res.dataset_measure == pytest.approx(measure_want, abs=5e-5)
        if plant:
            rc = res.correlations[:, ref.PLANT_CHANNEL]
            lag, i, j = np.unravel_index(np.nanargmax(rc), rc.shape)
            assert lag == 25 and i == j
            day = ref.Day(brain, audio, ref.PLANT_FS, keep=~detect_artifacts(brain, ref.PLANT_FS))
            assert np.allclose(res.correlations, day.correlations(), rtol=0, atol=1e-9, equal_nan=True)
