"""Host side of the spectrograms (Part 11 of include/dss_hip.h) without a GPU: declarations, argument checks and their reasons,
the window table, and the numpy restatement (tests/spectral_reference.py) held to tests/golden/spectral.npz, which
scipy.signal.spectrogram produced (tools/make_golden_spectral.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spectral_cases as sc
import spectral_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dss_spec_check_params", "dss_spec_trial_frames_for", "dss_spec_check_trials", "dss_spec_check_locked", "dss_spec_create",
       "dss_spec_destroy", "dss_spec_trials", "dss_spec_trials_dev", "dss_spec_locked", "dss_spec_locked_dev", "dss_spec_mean",
       "dss_spec_mean_dev", "dss_spec_geometry")


def test_entry_points_are_declared_and_exported():
    from dss_amd import _lib, spectral
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dss_hip.h")).read(), flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert re.search(r"#define\s+DSS_SPEC_PSD\s+0\b", text) and re.search(r"#define\s+DSS_SPEC_MAGNITUDE\s+1\b", text)
    assert spectral.MODES == {"psd": 0, "magnitude": 1}
    for name in ("hann_periodic", "SpectrogramGPU", "speech_locked_power", "geometry"):
        assert hasattr(spectral, name), name
    # the structure the Python side hands over is the header's: six ints and a double
    assert C.sizeof(spectral.SpecParams) == 32 and spectral.SpecParams.fs.offset == 24


def test_frame_counts_and_every_refusal():
    from dss_amd import _lib, spectral
    L = _lib.load()
    for n in range(50, 4100):
        assert L.dss_spec_trial_frames_for(n, 50, 10) == (n - 50) // 10 + 1
    assert [spectral.trial_frames(n, 50, 10) for n in (50, 59, 60, 210, 220, 380)] == [1, 1, 2, 17, 18, 34]
    assert spectral.trial_frames(16000, 800, 160) == 96
    assert spectral.trial_frames(2**40, 64, 64) == 2**34                             # 64-bit counts
    for n in (49, 1, 0, -5):
        assert L.dss_spec_trial_frames_for(n, 50, 10) == -1 and b"shorter than one window" in L.dss_last_error()
    assert spectral.check_trials(1000, [(0, 50), (60, 59), (130, 60), (200, 210), (400, 220), (620, 380)], 50, 10) == 73
    assert spectral.check_trials(1000, [], 50, 10) == 0

    def refused(message, fn, *args):
        with pytest.raises(_lib.DssError, match=message):
            fn(*args)
    refused("trial 1: 49 rows are shorter than one window", spectral.check_trials, 1000, [(0, 50), (100, 49)], 50, 10)
    refused("negative first row or length", spectral.check_trials, 1000, [(-1, 100)], 50, 10)
    refused("negative first row or length", spectral.check_trials, 1000, [(0, -100)], 50, 10)
    refused("trial 1 .* lies outside the signals", spectral.check_trials, 1000, [(0, 100), (901, 100)], 50, 10)
    refused("lies outside the signals", spectral.check_trials, 1000, [(10**15, 100)], 50, 10)
    refused("hop between frames must be at least 1", spectral.check_trials, 1000, [(0, 100)], 50, 0)
    refused("hop between frames must be at least 1", spectral.trial_frames, 100, 50, -3)
    refused("nperseg must be at least 2", spectral.trial_frames, 100, 1, 1)
    first = np.zeros(2, np.int64)
    length = np.full(2, 100, np.int64)
    assert L.dss_spec_check_trials(1000, 2, None, length.ctypes.data, 50, 10) == -1 and b"missing array" in L.dss_last_error()
    assert L.dss_spec_check_trials(1000, 2, first.ctypes.data, None, 50, 10) == -1 and b"missing array" in L.dss_last_error()
    assert L.dss_spec_check_trials(1000, -1, first.ctypes.data, length.ctypes.data, 50, 10) == -1 and b"negative count" in L.dss_last_error()
    big = np.full(1, 2**40, np.int64)
    assert L.dss_spec_check_trials(2**41, 1, first.ctypes.data, big.ctypes.data, 4, 1) == -1 and b"2^31 - 1 frames" in L.dss_last_error()

    # the onset-locked mean: trials of 380 and 220 rows have 34 and 18 frames
    ranges = [(620, 380), (400, 220)]
    assert spectral.check_locked(ranges, [3, 11], 3, 7, 50, 10) == 10
    assert spectral.check_locked(ranges, [27, 3], 3, 7, 50, 10) == 10                # onset + post == W is the last one allowed
    refused("trial 1: onset frame 2 has fewer than 3 frames before it", spectral.check_locked, ranges, [3, 2], 3, 7, 50, 10)
    refused("trial 0: onset frame 28 plus 7 frames runs past the trial's 34 frames", spectral.check_locked, ranges, [28, 3], 3, 7, 50, 10)
    refused("trial 1: onset frame 12 plus 7 frames runs past the trial's 18 frames", spectral.check_locked, ranges, [3, 12], 3, 7, 50, 10)
    refused("onset frame -1", spectral.check_locked, ranges, [3, -1], 0, 7, 50, 10)
    refused("shorter than one window", spectral.check_locked, [(0, 49)], [0], 0, 1, 50, 10)
    refused("frames before and", spectral.check_locked, ranges, [3, 3], -1, 7, 50, 10)
    refused("frames before and", spectral.check_locked, ranges, [3, 3], 0, 0, 50, 10)
    onset = np.zeros(2, np.int32)
    assert L.dss_spec_check_locked(2, None, onset.ctypes.data, 0, 1, 50, 10) == -1 and b"missing array" in L.dss_last_error()
    assert L.dss_spec_check_locked(2, length.ctypes.data, None, 0, 1, 50, 10) == -1 and b"missing array" in L.dss_last_error()
    assert L.dss_spec_check_locked(0, length.ctypes.data, onset.ctypes.data, 0, 1, 50, 10) == -1 and b"no trials" in L.dss_last_error()
    with pytest.raises(ValueError):
        spectral.check_locked(ranges, [3], 3, 7, 50, 10)

    P = spectral.SpecParams
    good = dict(nperseg=50, hop=10, nfft=100, mode=0, detrend=1, reserved=0, fs=1000.0)
    assert L.dss_spec_check_params(C.addressof(P(**good))) == 0
    for change in (dict(nfft=50), dict(nfft=2048), dict(nperseg=2048, nfft=2048, hop=2048), dict(nperseg=2, nfft=2, hop=1), dict(mode=1),
                   dict(detrend=0), dict(hop=10**6), dict(nfft=75)):
        assert L.dss_spec_check_params(C.addressof(P(**{**good, **change}))) == 0, change
    for change, message in ((dict(nfft=49), b"nfft (49) is smaller than nperseg (50)"), (dict(hop=0), b"hop between frames"),
                            (dict(hop=-10), b"hop between frames"), (dict(nperseg=1, nfft=1), b"nperseg must be at least 2"),
                            (dict(nfft=2049), b"up to 2048"), (dict(mode=2), b"unknown mode"), (dict(detrend=2), b"detrend"),
                            (dict(fs=0.0), b"sampling rate"), (dict(fs=float("nan")), b"sampling rate")):
        p = P(**{**good, **change})
        assert L.dss_spec_check_params(C.addressof(p)) == -1 and message in L.dss_last_error(), change
    assert L.dss_spec_check_params(None) == -1
    assert L.dss_spec_create(C.addressof(P(**{**good, "nfft": 49})), None) is None and b"nfft" in L.dss_last_error()
    # the handle forms refuse a missing handle instead of faulting
    assert L.dss_spec_trials(None, None, 0, 1, 1, 0, None, None, None) == -1
    assert L.dss_spec_trials_dev(None, None, 0, 1, 1, 0, None, None, None, None) == -1
    assert L.dss_spec_locked(None, None, 0, 1, 1, 0, None, None, None, 0, 1, None) == -1
    assert L.dss_spec_locked_dev(None, None, 0, 1, 1, 0, None, None, None, 0, 1, None, None) == -1
    assert L.dss_spec_mean(None, None, 0, 1, 1, 0, None, None, None) == -1
    assert L.dss_spec_mean_dev(None, None, 0, 1, 1, 0, None, None, None, None) == -1
    L.dss_spec_destroy(None)
    # the Python class refuses before it needs a device
    with pytest.raises(_lib.DssError, match="smaller than nperseg"):
        spectral.SpectrogramGPU(1000, 50, 40, nfft=49)
    with pytest.raises(_lib.DssError, match="hop between frames"):
        spectral.SpectrogramGPU(1000, 50, 50)
    with pytest.raises(ValueError):
        spectral.SpectrogramGPU(1000, 50, 40, mode="complex")
    assert spectral.locked_frame_counts() == (50, 150)


def test_hann_periodic_is_scipys_table_bit_for_bit():
    from scipy.signal import get_window
    from dss_amd.spectral import hann_periodic
    for n in (2, 50, 51, 800):
        got = hann_periodic(n)
        assert got.dtype == np.float64 and got.shape == (n,)
        assert np.array_equal(got, get_window("hann", n)), n


def test_restatement_equals_the_fixture_within_the_bound(golden):
    import scipy
    from dss_amd.spectral import hann_periodic
    g = golden("spectral.npz")
    if str(g["scipy_version"]) != scipy.__version__:
        print("fixture made with scipy", str(g["scipy_version"]), "- this machine has", scipy.__version__)
    fs, nperseg, noverlap, nfft = (int(v) for v in g["params"])
    x, ranges, want = g["signals"], [tuple(int(v) for v in r) for r in g["ranges"]], g["sxx"]
    n_ch = int(g["seed"][3])
    assert x.shape[1] == n_ch + 1 and want.shape == (73, n_ch, 51)
    assert g["frame_counts"].tolist() == [ref.frames_of(n, nperseg, nperseg - noverlap) for _, n in ranges] == [1, 1, 2, 17, 18, 34]
    spans = sorted((a, a + n) for a, n in ranges)
    assert any(a[1] > b[0] for a, b in zip(spans, spans[1:]))                       # two trials share rows
    assert np.array_equal(g["frequencies"], np.fft.rfftfreq(nfft, 1.0 / fs))
    # no frame is (nearly) constant: every frame's largest bin is at least 1e-6 of the case's mean largest bin
    peak = want.max(axis=-1)
    assert peak.min() >= 1e-6 * peak.mean()
    got = ref.trials(x[:, :n_ch], ranges, fs, hann_periodic(nperseg), nperseg, nperseg - noverlap, nfft)
    err = np.abs(got - want) / peak[..., None]
    print("restatement vs scipy, max |difference| / frame's largest bin:", err.max(), "bound", ref.frame_bound(np.ones(1), nperseg)[0])
    assert np.all(np.abs(got - want) <= ref.frame_bound(want, nperseg))             # every frame, channel and bin


def test_restatement_equals_scipy_in_the_other_modes():
    from scipy.signal import spectrogram
    from dss_amd.spectral import hann_periodic
    rng = np.random.default_rng(12)
    x = rng.standard_normal((700, 2)) + 0.5
    for nperseg, hop, nfft, mode, detrend in ((50, 10, 75, "psd", True), (64, 64, 64, "psd", True), (50, 10, 100, "psd", False),
                                              (80, 16, 80, "magnitude", True)):
        w = hann_periodic(nperseg)
        got = ref.spectrogram(x, 1000.0, w, nperseg, hop, nfft, mode, detrend)
        for c in range(2):
            _, _, sxx = spectrogram(x[:, c], fs=1000.0, window="hann", nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft, mode=mode,
                                    detrend="constant" if detrend else False)
            assert sxx.T.shape == got[:, c].shape
            assert np.all(np.abs(got[:, c] - sxx.T) <= ref.frame_bound(sxx.T, nperseg, mode)), (nperseg, hop, nfft, mode, detrend)


def test_without_a_device_the_compute_entry_points_say_so():
    from dss_amd import _lib, spectral
    L = _lib.load()
    if L.dss_device_count() > 0:
        return                                                                      # nothing to refuse where a device is present
    p = spectral.SpecParams(50, 10, 100, 0, 1, 0, 1000.0)
    win = spectral.hann_periodic(50)
    assert L.dss_spec_create(C.addressof(p), win.ctypes.data) is None
    assert b"no HIP device" in L.dss_last_error()
    with pytest.raises(_lib.DssError):
        spectral.SpectrogramGPU(1000, 50, 40, nfft=100)


# ---- which workgroup shape a call uses (dss_spec_geometry), and what tests/spectral_cases.py reaches with it --------------
SOFT, LIMIT = 80 * 1024, 160 * 1024                                                 # SPEC_LDS_SOFT and gfx950's LDS per workgroup


def test_case_list_reaches_every_workgroup_shape():
    """Keeps tests/test_gpu_spectral.py honest after any change to the picker: without a GPU, the case list reaches every F
    below 32 in all three kernels, a partial last group of bin blocks beside several channel groups in both reductions, and
    CG = 8 with a partial channel group."""
    from dss_amd.spectral import geometry
    seen_f = {k: set() for k in range(3)}
    tail_with_groups = {1: [], 2: []}
    cg8_partial = []
    print("case         kind    F CG  NB nblk  lds")
    for name, nperseg, hop, nfft, n_ch, mode, detrend in sc.CASES:
        for k, kind in enumerate(sc.KINDS):
            g = geometry(nperseg, hop, nfft, n_ch, kind, mode, "constant" if detrend else False)
            assert g == geometry(nperseg, hop, nfft, n_ch, k)                       # the kind by name or by number; mode and detrend do not matter
            print(f"{name:12s} {kind:6s} {g.F:2d} {g.CG:2d} {g.NB:3d} {g.nblk:4d} {g.lds_bytes:6d}")
            assert g.nblk == (nfft // 2 + 1 + 15) // 16
            assert g.F == sc.EXPECTED_F[name][k], (name, kind, g)
            seen_f[k].add(g.F)
            groups = -(-n_ch // g.CG)
            if k and g.nblk % g.NB and groups > 1:
                tail_with_groups[k].append(name)
            if g.CG == 8 and n_ch % 8:
                cg8_partial.append((name, kind))
    for k in range(3):
        assert seen_f[k] == {32, 16, 8, 4, 2, 1}, (sc.KINDS[k], seen_f[k])
    assert tail_with_groups[1] and tail_with_groups[2], tail_with_groups
    assert cg8_partial
    # what the table of the case list promises beyond F
    assert geometry(50, 10, 1000, 5, "trials")[:3] == (32, 8, 32)
    assert geometry(50, 10, 1100, 17, "trials")[:2] == (32, 16) and geometry(50, 10, 1100, 17, "locked")[:4] == (32, 1, 9, 35)
    assert geometry(2047, 2047, 2047, 2, "locked").lds_bytes == SOFT                # a request exactly at the limit is taken
    # the frame counts and windows of the case list against the F they are there for
    for name in sc.NAMES:
        F = sc.EXPECTED_F[name]
        W = sc.frames_per_trial(name)
        nperseg, hop = sc.params(name)[1:3]
        r = sc.ranges(name)
        assert [ref.frames_of(n, nperseg, hop) for _, n in r] == list(W)
        spans = sorted((a, a + n) for a, n in r)
        assert any(a[1] > b[0] for a, b in zip(spans, spans[1:]))                   # two trials share rows
        if name != "hopfar":
            for f in F:                                                             # per kernel: several tiles, a partial last one, a trial below F
                assert max(W) > f and (f == 1 or (any(w % f for w in W if w > f) and min(W) < f)), (name, f, W)
        if hop > 2:
            assert all((n - nperseg) % hop for _, n in r)                           # rows left behind the last frame
        lr, onsets, pre, post = sc.locked(name)
        assert len(lr) == len(onsets) >= 3 and all(o - pre >= 0 and o + post <= ref.frames_of(n, nperseg, hop) for (_, n), o in zip(lr, onsets))
        assert F[1] == 1 or (pre + post) % F[1], name
    assert any(sum(sc.locked(n)[2:]) < sc.EXPECTED_F[n][1] for n in sc.NAMES)
    assert any(sum(sc.locked(n)[2:]) > sc.EXPECTED_F[n][1] > 1 for n in sc.NAMES)


def test_picker_over_the_accepted_parameters():
    """Every accepted shape gets a cut that the kernels' index arithmetic and gfx950's LDS allow.  The finding the sweep
    records: no shape needs more than the preferred 80 KB, so the picker has one limit (spectrograms)."""
    from dss_amd import _lib
    from dss_amd.spectral import SpecParams
    L = _lib.load()
    out = (C.c_int * 5)()
    worst, n = (0, None), 0
    for nperseg in sorted(set(range(2, 2049, 37)) | {2047, 2048}):
        for nfft in sorted({nperseg, min(2 * nperseg, 2048), 2048}):
            for hop in sorted({1, max(1, nperseg // 4), nperseg, nperseg + 1, 10**6}):
                p = SpecParams(nperseg, hop, nfft, 0, 1, 0, 1000.0)
                nblk = (nfft // 2 + 1 + 15) // 16
                for n_ch in (1, 2, 3, 16, 17, 64):
                    cg_max = min(16, 1 << (n_ch - 1).bit_length())
                    for kind in range(3):
                        what = (nperseg, hop, nfft, n_ch, kind)
                        assert L.dss_spec_geometry(C.addressof(p), n_ch, kind, out) == 0, (what, L.dss_last_error())
                        F, CG, NB, blocks, lds = out
                        assert F in (1, 2, 4, 8, 16, 32) and CG in (1, 2, 4, 8, 16) and CG <= cg_max, (what, tuple(out))
                        assert blocks == nblk and 1 <= NB <= nblk and (kind or NB == nblk), (what, tuple(out))
                        assert 0 < lds <= LIMIT, (what, tuple(out))
                        worst = max(worst, (lds, what))
                        n += 1
    print(f"{n} shapes; the largest LDS request is {worst[0]} bytes at (nperseg, hop, nfft, C, kind) = {worst[1]}")
    assert n > 10000
    assert worst[0] <= SOFT                                                         # the finding: the preferred limit always suffices


def test_geometry_refuses_what_the_parameter_check_refuses():
    from dss_amd import _lib, spectral
    L = _lib.load()
    P = spectral.SpecParams
    good = dict(nperseg=50, hop=10, nfft=100, mode=0, detrend=1, reserved=0, fs=1000.0)
    out = (C.c_int * 5)()
    assert L.dss_spec_geometry(C.addressof(P(**good)), 128, 0, out) == 0 and tuple(out) == (32, 16, 4, 4, 52576)
    assert spectral.geometry(50, 10, 100, 128, "locked")[:4] == (32, 4, 4, 4) and spectral.geometry(50, 10, 100, 128, "mean")[:4] == (32, 2, 4, 4)
    for change, message in ((dict(nfft=49), b"nfft (49) is smaller than nperseg (50)"), (dict(hop=0), b"hop between frames"),
                            (dict(hop=-10), b"hop between frames"), (dict(nperseg=1, nfft=1), b"nperseg must be at least 2"),
                            (dict(nfft=2049), b"up to 2048"), (dict(mode=2), b"unknown mode"), (dict(detrend=2), b"detrend"),
                            (dict(fs=0.0), b"sampling rate"), (dict(fs=float("nan")), b"sampling rate")):
        p = P(**{**good, **change})
        assert L.dss_spec_check_params(C.addressof(p)) == -1
        want = L.dss_last_error()
        assert message in want
        for kind in range(3):
            assert L.dss_spec_geometry(C.addressof(p), 3, kind, out) == -1 and L.dss_last_error() == want, (change, kind)
    assert L.dss_spec_geometry(None, 3, 0, out) == -1 and b"no parameters" in L.dss_last_error()
    p = P(**good)
    for n_ch in (0, -1):
        assert L.dss_spec_geometry(C.addressof(p), n_ch, 0, out) == -1 and b"%d channels" % n_ch in L.dss_last_error()
    for kind in (-1, 3, 7):
        assert L.dss_spec_geometry(C.addressof(p), 3, kind, out) == -1 and b"unknown kernel kind %d" % kind in L.dss_last_error()
    assert L.dss_spec_geometry(C.addressof(p), 3, 0, None) == -1
    with pytest.raises(_lib.DssError, match="smaller than nperseg"):
        spectral.geometry(50, 10, 49, 3, "trials")
    with pytest.raises(_lib.DssError, match="0 channels"):
        spectral.geometry(50, 10, 100, 0, "mean")
    with pytest.raises(_lib.DssError, match="unknown kernel kind"):
        spectral.geometry(50, 10, 100, 3, 5)


@pytest.mark.parametrize("name", sc.NAMES)
def test_restatement_equals_scipy_on_the_case_list(name):
    """The reference against itself: tests/spectral_reference.py, which the GPU tests take the reductions' values and bounds
    from, agrees with scipy on every case of tests/spectral_cases.py, and no frame of a case is nearly silent."""
    from dss_amd.spectral import hann_periodic
    _, nperseg, hop, nfft, n_ch, mode, detrend = sc.params(name)
    x = sc.signals(name)
    assert x.dtype == np.float64 and x.shape[1] == n_ch and not x.flags.writeable
    want = sc.scipy_trials(name)
    got = ref.trials(x, sc.ranges(name), sc.FS, hann_periodic(nperseg), nperseg, hop, nfft, mode, detrend)
    assert got.shape == want.shape == (sum(sc.frames_per_trial(name)), n_ch, nfft // 2 + 1)
    peak = want.max(axis=-1)
    assert peak.min() >= 1e-6 * peak.mean()
    bound = ref.frame_bound(want, nperseg, mode)
    print(f"{name}: restatement vs scipy, max |difference| / bound {np.max(np.abs(got - want) / bound):.3g}")
    assert np.all(np.abs(got - want) <= bound)
