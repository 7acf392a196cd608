"""The spectrogram kernels (csrc/spectral.hip, Part 11 of include/dss_hip.h) on the GPU against scipy.signal.spectrogram: the
fixture tests/golden/spectral.npz (tools/make_golden_spectral.py), scipy called here for the other shapes, and the numpy
restatement (tests/spectral_reference.py) for the reductions.

Tolerance (derived, not measured): with n = nperseg, re and im are n-term sums of products of rounded factors, so
|dX| <= (n + 8) 2^-53 sum|seg| (the 8: detrend, window, table and scaling roundings), and by Parseval over the nfft bins
sum|seg| <= sqrt(n) max_k |X_k|.  Per frame: |dP[k]| <= 2 (n + 8) sqrt(n) 2^-53 max_k P[k] for the power density (9.1e-14 of
the frame's largest bin at n = 50, 5.1e-12 at n = 800), half that factor for the magnitude; for a mean of N frames the average
of the frames' bounds plus N 2^-53 |value|.  Every frame, channel and bin is compared.

Orders of the reductions, which the bit-for-bit tests restate on the host: `locked` adds the trials' frames in list order, from
0.0, and divides by the number of trials; `mean` adds every trial's frames in frame order, from 0.0, then the trials' sums in
list order, from 0.0, and divides by the number of frames.

The second half runs the cases of tests/spectral_cases.py: every workgroup shape the picker can choose (F below 32, a partial
last group of bin blocks beside several channel groups, CG = 8), with the same bounds.  tests/test_cpu_spectral.py proves
without a GPU that the list reaches those shapes; every test here asserts its case's shape first."""
import numpy as np
import pytest

import spectral_cases as sc
import spectral_reference as ref

pytestmark = pytest.mark.gpu

RANGES = [(0, 50), (60, 59), (130, 60), (200, 210), (400, 220), (620, 380)]


@pytest.fixture(scope="module")
def case(golden):
    g = golden("spectral.npz")
    fs, nperseg, noverlap, nfft = (int(v) for v in g["params"])
    assert (fs, nperseg, noverlap, nfft) == (1000, 50, 40, 100)
    assert [tuple(int(v) for v in r) for r in g["ranges"]] == RANGES
    x = g["signals"]
    x.setflags(write=False)
    return {"x": x, "sxx": g["sxx"], "bounds": np.concatenate([[0], np.cumsum(g["frame_counts"])])}


@pytest.fixture(scope="module")
def sp():
    from dss_amd.spectral import SpectrogramGPU
    s = SpectrogramGPU(1000, 50, 40, nfft=100)
    yield s
    s.close()


@pytest.fixture(scope="module")
def frames17(case, sp):
    """trials() of the fixture's list, 17 channels in rows of 18: computed once, shared, never written."""
    out = sp.trials(case["x"][:, :17], RANGES)
    out.setflags(write=False)
    return out


def _report(name, got, want, nperseg, mode="psd"):
    err = np.max(np.abs(got - want) / np.max(want, axis=-1, keepdims=True))
    print(f"{name}: max |difference| / frame's largest bin {err:.3g}, bound {ref.frame_bound(np.ones(1), nperseg, mode)[0]:.3g}")


def test_fixture_case_17_channels(case, sp, frames17):
    assert frames17.shape == (73, 17, 51) and frames17.dtype == np.float64
    assert np.array_equal(sp.frequencies, np.fft.rfftfreq(100, 1e-3)) and sp.trial_frames(380) == 34
    _report("nperseg 50 nfft 100 psd, C 17", frames17, case["sxx"], 50)
    assert np.all(np.abs(frames17 - case["sxx"]) <= ref.frame_bound(case["sxx"], 50))


def test_fixture_case_3_channels_and_strided_rows(case, sp, frames17):
    x = case["x"]
    got = sp.trials(np.ascontiguousarray(x[:, :4])[:, :3], RANGES)                   # C = 3 in rows of 4
    assert got.shape == (73, 3, 51)
    assert np.all(np.abs(got - case["sxx"][:, :3]) <= ref.frame_bound(case["sxx"][:, :3], 50))
    assert np.array_equal(got, frames17[:, :3])                                    # a channel's bits do not depend on its group
    # columns 5 .. 7 of the wide rows, and one channel given as a vector
    assert np.array_equal(sp.trials(x[:, 5:8], RANGES), frames17[:, 5:8])
    assert np.array_equal(sp.trials(x[:, 16], RANGES), frames17[:, 16:17])


def test_one_call_equals_one_call_per_trial_and_any_order(case, sp, frames17):
    x, b = case["x"][:, :17], case["bounds"]
    for k, r in enumerate(RANGES):
        assert np.array_equal(sp.trials(x, [r]), frames17[b[k]:b[k + 1]]), k
    rev = sp.trials(x, RANGES[::-1])
    pieces, at = [], 0
    for k in reversed(range(len(RANGES))):
        n = b[k + 1] - b[k]
        pieces.append((k, rev[at:at + n]))
        at += n
    assert at == len(rev)
    assert np.array_equal(np.concatenate([p for _, p in sorted(pieces, key=lambda kp: kp[0])]), frames17)
    assert sp.trials(x, []).shape == (0, 17, 51)


def test_torch_forms_equal_the_host_forms(case, sp, frames17):
    import torch
    d = torch.from_numpy(np.array(case["x"])).cuda()
    assert np.array_equal(sp.trials_torch(d[:, :17], RANGES).cpu().numpy(), frames17)
    onsets = [3, 11, 5]
    sub = [RANGES[5], RANGES[4], RANGES[3]]
    assert np.array_equal(sp.locked_torch(d[:, :17], sub, onsets, 3, 7).cpu().numpy(), sp.locked(case["x"][:, :17], sub, onsets, 3, 7))
    assert np.array_equal(sp.mean_torch(d[:, :17], RANGES).cpu().numpy(), sp.mean(case["x"][:, :17], RANGES))


def test_other_transform_lengths_against_scipy(case):
    from scipy.signal import spectrogram
    from dss_amd.spectral import SpectrogramGPU
    x = case["x"][:, :3]
    ranges = [(0, 50), (100, 333), (300, 700)]
    for nperseg, noverlap, nfft in ((50, 40, 75), (64, 0, 64)):                     # odd nfft: no doubled-Nyquist exception; hop = nperseg
        s = SpectrogramGPU(1000, nperseg, noverlap, nfft=nfft)
        got = s.trials(x, [r for r in ranges if r[1] >= nperseg])
        s.close()
        want = []
        for a, n in ranges:
            if n < nperseg:
                continue
            per = [spectrogram(x[a:a + n, c], fs=1000, window="hann", nperseg=nperseg, noverlap=noverlap, nfft=nfft)[2].T for c in range(3)]
            want.append(np.stack(per, axis=1))
        want = np.concatenate(want)
        assert got.shape == want.shape and want.shape[2] == nfft // 2 + 1
        _report(f"nperseg {nperseg} nfft {nfft} psd", got, want, nperseg)
        assert np.all(np.abs(got - want) <= ref.frame_bound(want, nperseg)), (nperseg, nfft)


def test_frames_that_do_not_overlap_and_a_long_transform(case):
    """The two other paths of the kernels, against the restatement: hop > nperseg (every frame is staged on its own), and
    nfft = 2048 (1025 bins: the reductions split the bin blocks over several workgroups)."""
    from dss_amd.spectral import SpectrogramGPU, hann_periodic
    x = case["x"][:, :3]
    ranges = [(5, 50), (100, 333), (300, 700)]
    s = SpectrogramGPU(1000, 50, -30, nfft=64)                                       # hop 80
    got = s.trials(x, ranges)
    s.close()
    want = ref.trials(x, ranges, 1000, hann_periodic(50), 50, 80, 64)
    assert got.shape == want.shape == (1 + 4 + 9, 3, 33)
    assert np.all(np.abs(got - want) <= ref.frame_bound(want, 50))

    x, ranges, onsets = case["x"][:, 2], [(100, 333), (300, 700), (5, 150)], [1, 7, 0]
    s = SpectrogramGPU(1000, 100, 50, nfft=2048)
    frames = s.trials(x, ranges)
    locked, mean = s.locked(x, ranges, onsets, 0, 2), s.mean(x, ranges)
    s.close()
    want = ref.trials(x, ranges, 1000, hann_periodic(100), 100, 50, 2048)
    assert frames.shape == want.shape == (5 + 13 + 2, 1, 1025)
    assert np.all(np.abs(frames - want) <= ref.frame_bound(want, 100))
    at = [0, 5, 18, 20]
    acc = np.zeros((2, 1, 1025))
    for k, o in enumerate(onsets):
        acc = acc + frames[at[k] + o:at[k] + o + 2]
    assert np.array_equal(locked, (acc / 3).transpose(1, 2, 0))
    total = np.zeros((1, 1025))
    for k in range(3):
        part = np.zeros((1, 1025))
        for f in range(at[k], at[k + 1]):
            part = part + frames[f]
        total = total + part
    assert np.array_equal(mean, total / 20)


def test_magnitude_of_int16_audio_against_scipy():
    from scipy.signal import spectrogram
    from dss_amd.spectral import SpectrogramGPU
    from dss_amd.synthetic import synthetic_speech_audio
    wav = synthetic_speech_audio(31, 16000, 16000)
    assert wav.dtype == np.int16 and len(wav) == 16000
    s = SpectrogramGPU(16000, 800, 640, mode="magnitude")
    got = s.trials(wav, [(0, 16000)])
    s.close()
    _, _, want = spectrogram(wav.astype(np.float64), fs=16000, window="hann", nperseg=800, noverlap=640, mode="magnitude")
    want = want.T[:, None, :]
    assert got.shape == want.shape == (96, 1, 401)
    peak = want.max(axis=-1)
    assert peak.min() >= 1e-6 * peak.mean()                                         # no frame is (nearly) silent
    _report("nperseg 800 magnitude, int16", got, want, 800, "magnitude")
    assert np.all(np.abs(got - want) <= ref.frame_bound(want, 800, "magnitude"))


def test_detrend_off_against_the_restatement(case):
    from dss_amd.spectral import SpectrogramGPU, hann_periodic
    x = case["x"][:, :3]
    s = SpectrogramGPU(1000, 50, 40, nfft=100, detrend=False)
    got = s.trials(x, RANGES)
    s.close()
    want = ref.trials(x, RANGES, 1000, hann_periodic(50), 50, 10, 100, detrend=False)
    assert np.all(np.abs(got - want) <= ref.frame_bound(want, 50))
    # the mean matters: the drifting signals' bin 0 differs from the detrended one
    detrended = ref.trials(x, RANGES, 1000, hann_periodic(50), 50, 10, 100)
    assert np.max(np.abs(want - detrended) / ref.frame_bound(want, 50)) > 1e6


def test_locked_mean(case, sp, frames17):
    from dss_amd.spectral import hann_periodic
    x, b = case["x"][:, :17], case["bounds"]
    # six trials with different onsets; the list repeats ranges, which is as good as overlap
    order = [5, 4, 3, 5, 3, 4]
    onsets = [3, 11, 5, 27, 10, 4]
    sub = [RANGES[k] for k in order]
    got = sp.locked(x, sub, onsets, 3, 7)
    assert got.shape == (17, 51, 10)
    want, bound = ref.locked(x, sub, onsets, 3, 7, 1000, hann_periodic(50), 50, 10, 100)
    print("locked: max |difference| / bound", np.max(np.abs(got - want) / bound))
    assert np.all(np.abs(got - want) <= bound)
    # the kernel's order: the trials' frames added in list order from 0.0, then divided by the number of trials
    acc = np.zeros((10, 17, 51))
    for k, o in zip(order, onsets):
        acc = acc + frames17[b[k] + o - 3:b[k] + o + 7]
    assert np.array_equal(got, (acc / len(order)).transpose(1, 2, 0))
    # one trial: the frames themselves
    assert np.array_equal(sp.locked(x, [RANGES[5]], [20], 20, 14), frames17[b[5]:b[6]].transpose(1, 2, 0))


def test_mean_spectrum(case, sp, frames17):
    from dss_amd.spectral import hann_periodic
    x, b = case["x"][:, :17], case["bounds"]
    got = sp.mean(x, RANGES)
    assert got.shape == (17, 51)
    want, bound = ref.mean(x, RANGES, 1000, hann_periodic(50), 50, 10, 100)
    print("mean: max |difference| / bound", np.max(np.abs(got - want) / bound))
    assert np.all(np.abs(got - want) <= bound)
    # the kernel's order: every trial's frames in frame order from 0.0, the trials' sums in list order from 0.0, / frames
    total = np.zeros((17, 51))
    for k in range(len(RANGES)):
        part = np.zeros((17, 51))
        for f in range(b[k], b[k + 1]):
            part = part + frames17[f]
        total = total + part
    assert np.array_equal(got, total / 73)
    assert np.array_equal(sp.mean(x[:, :3], RANGES), got[:3])


def test_speech_locked_power():
    from dss_amd.spectral import speech_locked_power
    rng = np.random.default_rng(77)
    n_ch = 20
    cal = rng.standard_normal((9000, n_ch)) * (1.0 + 0.1 * np.arange(n_ch))
    rec = rng.standard_normal((24000, n_ch)) * (1.0 + 0.1 * np.arange(n_ch))
    rec[:, ::3] += 2.0 * np.sin(2 * np.pi * 90.0 * np.arange(24000) / 1000.0)[:, None]
    cal_ranges = [(1000 * k + 17 * k, 700 + 30 * k) for k in range(8)]
    ranges = [(2900 * k + 11 * k, 2400 + 60 * k) for k in range(8)]                 # 236 .. 278 frames each
    onsets = [50 + 4 * k for k in range(8)]                                         # 50 frames before, 150 after fit every trial
    got = speech_locked_power(cal, cal_ranges, rec, ranges, onsets)
    want, ratio = ref.speech_locked_power(cal, cal_ranges, rec, ranges, onsets)
    assert got.shape == want.shape == (n_ch, 51, 200) and got.dtype == np.float32
    assert 1e-3 <= ratio.min() and ratio.max() <= 1e3
    print("speech_locked_power: max |difference| in dB", np.max(np.abs(got.astype(np.float64) - want)), "ratios", ratio.min(), ratio.max())
    assert np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))) <= 1e-4
    import torch
    dev = speech_locked_power(torch.from_numpy(cal).cuda(), cal_ranges, torch.from_numpy(rec).cuda(), ranges, onsets)
    assert np.array_equal(dev, got)


# ---- every workgroup shape the picker can choose (tests/spectral_cases.py) -----------------------------------------------
@pytest.fixture(scope="module", params=sc.NAMES)
def shaped(request):
    """One case: its handle, signals, trial list, trials() of the whole list (computed once, shared, never written) and where
    each trial's frames start in it."""
    from dss_amd.spectral import SpectrogramGPU
    name = request.param
    _, nperseg, hop, nfft, n_ch, mode, detrend = sc.params(name)
    s = SpectrogramGPU(sc.FS, nperseg, nperseg - hop, nfft=nfft, mode=mode, detrend="constant" if detrend else False)
    x, ranges = sc.signals(name), sc.ranges(name)
    frames = s.trials(x, ranges)
    frames.setflags(write=False)
    at = np.concatenate([[0], np.cumsum([ref.frames_of(n, nperseg, hop) for _, n in ranges])])
    yield {"name": name, "sp": s, "x": x, "ranges": ranges, "frames": frames, "at": at, "ref": (sc.FS, s.window, nperseg, hop, nfft, mode, detrend)}
    s.close()


def _assert_shape(name):
    """The case still runs the workgroup shape it is named for: otherwise the test no longer tests what it says."""
    from dss_amd.spectral import geometry
    _, nperseg, hop, nfft, n_ch, mode, detrend = sc.params(name)
    got = tuple(geometry(nperseg, hop, nfft, n_ch, kind, mode, "constant" if detrend else False).F for kind in sc.KINDS)
    assert got == sc.EXPECTED_F[name], (name, got)


def test_shapes_trials_against_scipy(shaped):
    name, frames = shaped["name"], shaped["frames"]
    _assert_shape(name)
    _, nperseg, hop, nfft, n_ch, mode, _ = sc.params(name)
    want = sc.scipy_trials(name)
    assert frames.shape == want.shape == (shaped["at"][-1], n_ch, nfft // 2 + 1) and frames.dtype == np.float64
    _report(f"{name} trials", frames, want, nperseg, mode)
    assert np.all(np.abs(frames - want) <= ref.frame_bound(want, nperseg, mode))    # every frame, channel and bin


def test_shapes_locked_and_mean(shaped):
    name, sp, x, frames, at = (shaped[k] for k in ("name", "sp", "x", "frames", "at"))
    _assert_shape(name)
    lr, onsets, pre, post = sc.locked(name)
    got = sp.locked(x, lr, onsets, pre, post)
    want, bound = ref.locked(x, lr, onsets, pre, post, *shaped["ref"])
    assert got.shape == want.shape
    print(f"{name} locked: max |difference| / bound {np.max(np.abs(got - want) / bound):.3g}")
    assert np.all(np.abs(got - want) <= bound)
    # the kernel's order, on frames that another workgroup shape computed: list order from 0.0, then / trials
    acc = np.zeros((pre + post,) + frames.shape[1:])
    for r, o in zip(lr, onsets):
        k = shaped["ranges"].index(r)
        acc = acc + frames[at[k] + o - pre:at[k] + o + post]
    assert np.array_equal(got, (acc / len(lr)).transpose(1, 2, 0))

    got = sp.mean(x, shaped["ranges"])
    want, bound = ref.mean(x, shaped["ranges"], *shaped["ref"])
    assert got.shape == want.shape
    print(f"{name} mean: max |difference| / bound {np.max(np.abs(got - want) / bound):.3g}")
    assert np.all(np.abs(got - want) <= bound)
    # frames in order from 0.0, then the trials' sums in list order from 0.0, then / frames
    total = np.zeros(frames.shape[1:])
    for k in range(len(at) - 1):
        part = np.zeros(frames.shape[1:])
        for f in range(at[k], at[k + 1]):
            part = part + frames[f]
        total = total + part
    assert np.array_equal(got, total / at[-1])


def test_shapes_locked_of_one_trial_is_its_frames(shaped):
    name, sp, x, frames, at = (shaped[k] for k in ("name", "sp", "x", "frames", "at"))
    _assert_shape(name)
    for k, r in enumerate(shaped["ranges"]):
        W = at[k + 1] - at[k]
        for pre in sorted({0, W // 2}):                                             # the onset does not matter, only onset - pre
            assert np.array_equal(sp.locked(x, [r], [pre], pre, W - pre), frames[at[k]:at[k + 1]].transpose(1, 2, 0)), (k, pre)


def test_shapes_channels_do_not_depend_on_their_group(shaped):
    name, sp, x, frames = (shaped[k] for k in ("name", "sp", "x", "frames"))
    _assert_shape(name)
    n_ch = x.shape[1]
    for cols in (slice(1, None, 2), slice(n_ch - 2, n_ch), slice(None, None, 3)):    # copied; read in place from the wide rows; copied
        assert np.array_equal(sp.trials(x[:, cols], shaped["ranges"]), frames[:, cols]), cols
    assert np.array_equal(sp.trials(x[:, n_ch - 1], shaped["ranges"]), frames[:, n_ch - 1:])
    assert np.array_equal(sp.mean(x[:, 1::2], shaped["ranges"]), sp.mean(x, shaped["ranges"])[1::2])


def test_shapes_lists_do_not_matter(shaped):
    name, sp, x, frames, at, ranges = (shaped[k] for k in ("name", "sp", "x", "frames", "at", "ranges"))
    _assert_shape(name)
    for k, r in enumerate(ranges):
        assert np.array_equal(sp.trials(x, [r]), frames[at[k]:at[k + 1]]), k
    rev = sp.trials(x, ranges[::-1])
    assert len(rev) == len(frames)
    pos = 0
    for k in reversed(range(len(ranges))):
        n = at[k + 1] - at[k]
        assert np.array_equal(rev[pos:pos + n], frames[at[k]:at[k + 1]]), k
        pos += n
