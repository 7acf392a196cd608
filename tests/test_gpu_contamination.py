"""The correlation kernels of the acoustic contamination analysis (csrc/contamination.hip, Part 12 of include/dss_hip.h) on the
GPU against the float64 statement of the method (tests/contamination_reference.py).  Every sum and every finite correlation is
compared within the bound that module derives (the DFT's n-term sums, propagated through the P-term sums into r to first order);
each case prints max |difference| / bound.  The shapes are the smallest that reach every path: 121 frames at the default operator
(three full tiles of 32 and a partial one; 51 lags in two lag groups of the grid, whose waves hold 7, 7, 7, 7 and 7, 7, 7, 2 lags), 3 and 17
channels, frames masked inside, at a tile edge and at both ends; a small operator whose lags cross tile edges and leave waves
with fewer lags than their share, or none; fewer frames than lags; a constant channel.

The case table of tests/contamination_cases.py goes through the same comparison: chunks of several tiles with a shorter last
chunk, one chunk for everything, the mask in every place it can ride in, the DC and Nyquist bins, odd, abutting and apart
windows, one to three lag groups, lags beyond the recording, full and one-frame tiles, no, one and a few kept frames, the largest
window the LDS holds.  Each of them asserts the launch plan it is there to reach (``ContaminationGPU.plan``) before it runs.
Beside the bounds: what must hold bit for bit (empty lags, powers of two, an all-zero channel, a handle reused across sizes, a
side stream, CUDA tensors through the whole analysis)."""
import numpy as np
import pytest

import contamination_cases as cases
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


def _inputs(name):
    return cases.build(name) if name in cases.NAMES else _case(name)


def _fresh(name):
    """The library's sums of a case from host buffers on a handle of its own; a case of the table first asserts that the
    library plans the launch the case is there to reach."""
    from dss_amd.contamination import ContaminationGPU
    op, brain, audio, keep = _inputs(name)
    g = ContaminationGPU(**op)
    try:
        if name in cases.NAMES:
            assert g.plan(len(brain), brain.shape[1]) == cases.spec(name).plan, name
        m = g.moments(brain, audio, keep)
        shape = (g.nperseg, g.hop, g.bin_lo, g.n_bins, g.max_lag, g.frames(len(brain)))
    finally:
        g.close()
    for v in m:
        v.setflags(write=False)
    return m, shape


class _Results(dict):
    """name -> (the library's sums, the reference's spectrograms, the shape): each case once, when first asked for.  Shared,
    never written."""

    def __missing__(self, name):
        m, shape = _fresh(name)
        if name in cases.NAMES:
            day = cases.day(name)
        else:
            op, brain, audio, keep = _case(name)
            day = ref.Day(brain, audio, keep=keep, **op)
        self[name] = (m, day, shape)
        return self[name]


@pytest.fixture(scope="module")
def results():
    return _Results()


def _within_bounds(name, m, day):
    """The library's sums `m` against the reference's spectrograms `day`: n equal, the five sums within their derived bounds, the
    NaN pattern of r equal, r within its bound and the bound small; prints max |difference| / bound."""
    from dss_amd.contamination import correlations_from_moments
    # the shift is the mean of the kept audio frames, to rounding; the reference takes the library's value as it is
    if day.fm.any():
        assert np.allclose(m.shift, day.A[day.fm].mean(axis=0), rtol=1e-12, atol=0)
    else:
        assert np.array_equal(m.shift, np.zeros(len(day.bins)))
    want, bound = day.moments(m.shift)
    assert np.array_equal(m.n, want["n"])
    for key in NAMES[1:]:
        got = getattr(m, key)
        assert got.shape == want[key].shape, key
        live = bound[key] > 0
        assert np.array_equal(live, np.broadcast_to(want["n"].reshape((-1,) + (1,) * (got.ndim - 1)) > 0, got.shape)), key
        if live.any():
            print(f"{name} {key}: max |difference| / bound {np.max(np.abs(got - want[key])[live] / bound[key][live]):.3g}")
        assert np.all(np.abs(got - want[key]) <= bound[key]), key                       # a NaN fails; an empty lag must be exactly 0
    r, r_want = correlations_from_moments(m), day.correlations()
    assert r.shape == r_want.shape == (2 * day.L + 1, day.N.shape[1], len(day.bins), len(day.bins))
    assert np.array_equal(np.isnan(r), np.isnan(r_want))                               # nothing skipped that the reference defines
    ok = ~np.isnan(r_want)
    assert ok.any() == (name not in cases.NO_CORRELATION)
    if ok.any():
        rb = ref.r_bound(want, bound)
        print(f"{name} r: max |difference| / bound {np.max(np.abs(r - r_want)[ok] / rb[ok]):.3g}, largest bound {np.max(rb[ok]):.3g}")
        assert np.all(np.abs(r - r_want)[ok] <= rb[ok]) and np.median(rb[ok]) < 1e-9         # and the bound says something
    return r


@pytest.mark.parametrize("name", CASES + cases.NAMES)
def test_sums_and_correlations_within_the_derived_bounds(results, name):
    m, day, shape = results[name]
    assert shape == (day.nperseg, day.hop, int(day.bins[0]), len(day.bins), day.L, day.W)
    if name.startswith("default_c"):
        assert shape == (200, 20, 14, 21, 25, 121)
    if name == "small_operator":
        assert shape == (16, 4, 2, 4, 3, 40)
    if name in cases.NAMES:
        assert shape == cases.spec(name).shape
    r = _within_bounds(name, m, day)
    if name in cases.NAMES:
        assert all(np.isfinite(v).all() for v in m)                                    # apart: no row between the frames was read
        cases.check_exact(name, m.n, m.shift, m._asdict(), r)


def test_empty_lags_and_recordings_without_pairs_are_exact(results):
    """No tolerance: a lag without pairs is n = 0 and zeros, whether the frames are dropped or the lag is longer than the
    recording; one kept frame pairs with itself at lag 0 only."""
    from dss_amd.contamination import correlations_from_moments
    m, _, _ = results["keep_none"]
    for key in m._fields:
        assert np.array_equal(getattr(m, key), np.zeros_like(getattr(m, key))), key    # the shift too
    assert np.all(np.isnan(correlations_from_moments(m)))
    m, day, _ = results["keep_one"]
    assert list(m.n) == [0, 0, 0, 1, 0, 0, 0] and int(day.fm.sum()) == 1 and np.all(np.isnan(correlations_from_moments(m)))
    for key in NAMES[1:]:
        assert not np.delete(getattr(m, key), 3, axis=0).any(), key
    assert np.array_equal(m.sa[3], np.zeros(4)) and np.array_equal(m.saa[3], np.zeros(4))          # the one frame is its own mean
    assert np.array_equal(m.sab[3], np.zeros((2, 4, 4))) and np.all(m.sb[3] > 0) and np.array_equal(m.sbb[3], m.sb[3] ** 2)
    m, day, _ = results["largest_lag"]
    assert day.W == 40 and day.L == 4096 and len(m.n) == 8193
    far = np.abs(np.arange(-4096, 4097)) >= 40
    assert far.sum() == 8193 - 79 and not m.n[far].any() and m.n[~far].all()
    for key in NAMES[1:]:
        assert np.array_equal(getattr(m, key)[far], np.zeros_like(getattr(m, key)[far])), key
    assert np.all(np.isnan(correlations_from_moments(m)[far]))


def _equal(a, b, keys=None):
    for key in keys or a._fields:
        assert np.array_equal(getattr(a, key), getattr(b, key)), key


def test_powers_of_two_scale_the_sums_bit_for_bit(results):
    """many_tiles (chunks of 3 tiles): a power of two on either side changes exponents only, in every sum it enters."""
    from dss_amd.contamination import ContaminationGPU
    op, brain, audio, keep = cases.build("many_tiles")
    m = results["many_tiles"][0]
    g = ContaminationGPU(**op)
    try:
        for k in (40, -40):
            s = g.moments(brain * 2.0 ** k, audio, keep)
            _equal(s, m, ("n", "shift", "sa", "saa"))
            assert np.array_equal(s.sb, m.sb * 2.0 ** k) and np.array_equal(s.sbb, m.sbb * 2.0 ** (2 * k)), k
            assert np.array_equal(s.sab, m.sab * 2.0 ** k), k
        for k in (30, -30):
            s = g.moments(brain, audio * 2.0 ** k, keep)
            _equal(s, m, ("n", "sb", "sbb"))
            assert np.array_equal(s.shift, m.shift * 2.0 ** k) and np.array_equal(s.sa, m.sa * 2.0 ** k), k
            assert np.array_equal(s.saa, m.saa * 2.0 ** (2 * k)) and np.array_equal(s.sab, m.sab * 2.0 ** k), k
    finally:
        g.close()
    assert m.sab.all() and m.sbb.all() and m.saa.all()                                  # nothing compared was a zero


def test_an_all_zero_channel_is_exactly_zero_and_leaves_its_neighbours_bits_alone(results):
    from dss_amd.contamination import ContaminationGPU, correlations_from_moments
    op, brain, audio, keep = cases.build("many_tiles")
    silent = brain.copy()
    silent[:, 7] = 0.0
    others = np.delete(np.arange(40), 7)
    g = ContaminationGPU(**op)
    try:
        assert g.plan(len(brain), 39)[1:] == g.plan(len(brain), 40)[1:] == cases.spec("many_tiles").plan[1:]   # the same cut
        with_it = g.moments(silent, audio, keep)
        without = g.moments(np.ascontiguousarray(brain[:, others]), audio, keep)
    finally:
        g.close()
    assert not with_it.sb[:, 7].any() and not with_it.sbb[:, 7].any() and not with_it.sab[:, 7].any()
    r = correlations_from_moments(with_it)
    assert np.all(np.isnan(r[:, 7])) and not np.isnan(r[:, others]).any()
    _equal(with_it, without, ("n", "shift", "sa", "saa"))
    for key in ("sb", "sbb", "sab"):
        assert np.array_equal(getattr(with_it, key)[:, others], getattr(without, key)), key
        assert np.array_equal(getattr(with_it, key)[:, others], getattr(results["many_tiles"][0], key)[:, others]), key


def _cuda(a):
    """A host array as a CUDA tensor with the same strides (a column slice stays a view of its wider rows)."""
    import torch
    if a.ndim == 2 and a.base is not None and a.strides[0] != 8 * a.shape[1]:
        first = (a.__array_interface__["data"][0] - a.base.__array_interface__["data"][0]) // 8
        assert a.base.ndim == 2 and 0 < first < a.base.shape[1]
        view = torch.from_numpy(np.array(a.base)).cuda()[:, first:first + a.shape[1]]
        assert view.stride() == (a.strides[0] // 8, 1)
        return view
    return torch.from_numpy(np.array(a)).cuda()


def test_one_handle_reused_across_sizes_gives_a_fresh_handles_bits(results):
    """The workspaces of a handle grow and are kept: a long recording, one frame, nothing kept, 520 strided channels in one
    chunk, the long recording again, host and device forms in turn."""
    import torch
    from dss_amd.contamination import ContaminationGPU, Moments
    g = ContaminationGPU(**cases.SMALL)
    try:
        for k, name in enumerate(("many_tiles", "frames_1", "keep_none", "one_chunk", "many_tiles")):
            op, brain, audio, keep = cases.build(name)
            assert op == cases.SMALL
            if k % 2 == 0:
                m = g.moments(brain, audio, keep)
            else:
                dev = g.moments_torch(_cuda(brain), _cuda(audio), keep)
                torch.cuda.synchronize()
                m = Moments(*[v.cpu().numpy() for v in dev])
            _equal(m, results[name][0])
        op, brain, audio, keep = cases.build("many_tiles")
        dev = g.moments_torch(_cuda(brain), _cuda(audio), keep)                        # and the device form of the long one
        _equal(Moments(*[v.cpu().numpy() for v in dev]), results["many_tiles"][0])
    finally:
        g.close()


def test_a_side_stream_gives_the_default_streams_bits(results):
    import torch
    from dss_amd.contamination import ContaminationGPU, Moments
    op, brain, audio, keep = cases.build("many_tiles")
    side = torch.cuda.Stream()
    hb, ha = torch.from_numpy(np.array(brain) / 2).cuda(), torch.from_numpy(np.array(audio) / 2).cuda()
    torch.cuda.synchronize()
    g = ContaminationGPU(**op)
    try:
        with torch.cuda.stream(side):
            db, da = hb * 2, ha * 2                                                    # the inputs are produced on the side stream
        dev = g.moments_torch(db, da, keep, stream=side.cuda_stream)
        side.synchronize()
        _equal(Moments(*[v.cpu().numpy() for v in dev]), results["many_tiles"][0])
        with torch.cuda.stream(side):                                                  # stream=None: the current stream
            dev = g.moments_torch(db, da, keep)
        side.synchronize()
        _equal(Moments(*[v.cpu().numpy() for v in dev]), results["many_tiles"][0])
    finally:
        g.close()


def test_the_analysis_of_cuda_tensors_equals_that_of_host_arrays():
    import torch
    from dss_amd.contamination import contamination_analysis
    brain, audio = ref.planted_case(True)
    host = contamination_analysis(brain, audio, ref.PLANT_FS, n_surrogates=500)
    dev = contamination_analysis(torch.from_numpy(brain).cuda(), torch.from_numpy(audio).cuda(), ref.PLANT_FS, n_surrogates=500)
    assert host.criterion_value < 0.05 and not np.isnan(host.correlations).all()
    for key in host._fields:
        a, b = np.asarray(getattr(host, key)), np.asarray(getattr(dev, key))
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), key


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
