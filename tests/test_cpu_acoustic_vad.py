"""Host side of the acoustic VAD labels (Part 7 of include/dss_hip.h) without a GPU: tables, argument checks, the threshold /
vote of one trial and the session arithmetic, held to tests/golden/acoustic_vad.npz, which the reference's own
EnergyBasedVad / MelFilterBank produced (tools/make_golden_acoustic_vad.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import acoustic_vad_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dss_avad_check_params", "dss_avad_create", "dss_avad_destroy", "dss_avad_trial_frames_for", "dss_avad_check_trials",
       "dss_avad_labels_trials", "dss_avad_labels_trials_dev", "dss_avad_vote_host")


def _trials(g):
    bounds = np.concatenate([[0], np.cumsum(g["frame_counts"])])
    return [(int(f), int(n), int(lead), bool(s), int(a), int(b)) for (f, n, lead, s), a, b in zip(g["trials"], bounds, bounds[1:])]


def _audio(g):
    import hashlib
    from dss_amd.synthetic import synthetic_speech_audio
    seed, n, fs, z0, z1 = (int(v) for v in g["audio_seed"])
    wav = synthetic_speech_audio(seed, n, fs)
    wav[z0:z1] = 0
    assert hashlib.sha256(wav.tobytes()).digest() == g["audio_sha"].tobytes()
    return wav


def test_entry_points_are_declared_and_exported():
    from dss_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dss_hip.h")).read(), flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name


def test_fixture_covers_the_edge_cases(golden):
    g = golden("acoustic_vad.npz")
    prov = str(g["provenance"])
    assert "reference classes" in prov and "h5py placeholder untouched" in prov and "hanning" in prov
    t = _trials(g)
    lengths = [n for _, n, _, _, _, _ in t]
    assert 800 in lengths and 960 in lengths and any(abs(n - 40640) < 10 for n in lengths) and any(abs(n - 64640) < 10 for n in lengths)
    assert g["frame_counts"].tolist() == [ref.frames_of(n) for n in lengths]
    spans = sorted((f, f + n - lead) for f, n, lead, _, _, _ in t)
    assert any(a[1] > b[0] for a, b in zip(spans, spans[1:]))                       # two trials share samples
    assert any(n < asked for (_, asked), n in zip(g["trials_asked"], lengths))      # one was clamped at the end of the audio
    assert max(f + n - lead for f, n, lead, _, _, _ in t) <= int(g["audio_seed"][1])
    sil = [x for x in t if x[3]]
    assert len(sil) == 1 and not g["labels"][sil[0][4]:sil[0][5]].any()
    le = g["log_energy"][sil[0][4]:sil[0][5]]
    assert (le > g["thresholds"][t.index(sil[0])]).sum() > 10                      # ... although it holds speech
    flat = [x for x in t if np.all(g["log_energy"][x[4]:x[5]] == 2 * 40 * np.log(1e-7))]
    assert len(flat) == 1 and not g["labels"][flat[0][4]:flat[0][5]].any()          # digital silence
    assert g["labels"].any() and not g["labels"].all()
    # no frame lies near its trial's threshold, so labels can be compared frame by frame whatever the summation order
    for k, x in enumerate(t):
        assert np.min(np.abs(g["log_energy"][x[4]:x[5]] - g["thresholds"][k])) >= 0.8, k


def test_tables_equal_the_reference_class(golden):
    from dss_amd import acoustic_vad
    g = golden("acoustic_vad.npz")
    got = acoustic_vad.mel_filterbank(401, 40, 16000)
    want = g["mel"]
    assert got.shape == want.shape == (401, 40) and got.dtype == np.float64
    assert np.array_equal(got != 0, want != 0)                                      # same zero pattern, hence the same band edges
    assert [np.nonzero(got[:, b])[0][[0, -1]].tolist() for b in range(40)] == [np.nonzero(want[:, b])[0][[0, -1]].tolist() for b in range(40)]
    # same operations in the same order (ramp / width, divided by the band's own numpy sum): bit for bit
    assert np.array_equal(got, want)
    assert np.array_equal(acoustic_vad.hann(800), g["window"])                      # numpy.hanning on both sides: bit for bit


def test_vote_host_gives_the_reference_labels(golden):
    from dss_amd import acoustic_vad
    g = golden("acoustic_vad.npz")
    for k, (_, n, _, silence, a, b) in enumerate(_trials(g)):
        labels, thr = acoustic_vad.vote_host(g["log_energy"][a:b])
        if silence:
            labels = np.zeros_like(labels)
        assert np.array_equal(labels, g["labels"][a:b]), k
        assert abs(thr - g["thresholds"][k]) <= 1e-12 * abs(g["thresholds"][k]), k
    # the reference's loop, restated, on other parameters and random energies
    rng = np.random.default_rng(5)
    for ctx, prop, scale, thr0 in ((0, 0.6, 1.0, 4.0), (8, 0.3, 1.0, 4.0), (5, 0.6, 0.0, -2.0), (1, 0.99, 2.5, -3.0), (3, 0.5, 1.0, 0.0)):
        for W in (1, 2, 3, 9, 10, 11, 255, 256, 257, 700):
            le = rng.standard_normal(W) * 6.0 - 3.0
            got, thr = acoustic_vad.vote_host(le, thr0, scale, ctx, prop)
            want, wthr, gap = ref.vote(le, thr0, scale, ctx, prop)
            assert abs(thr - wthr) <= 1e-12 * max(abs(wthr), 1.0)
            if gap > 1e-9:
                assert np.array_equal(got, want), (ctx, prop, scale, thr0, W)


def test_restatement_agrees_with_the_reference(golden):
    g = golden("acoustic_vad.npz")
    wav = _audio(g)
    worst = 0.0
    for k, (first, n, lead, silence, a, b) in enumerate(_trials(g)):
        le = ref.log_energy(ref.trial_samples(wav, first, n, lead), g["window"], g["mel"])
        worst = max(worst, float(np.max(np.abs(le - g["log_energy"][a:b]))))
        labels, thr, _ = ref.vote(le)
        if silence:
            labels[:] = False
        assert np.array_equal(labels, g["labels"][a:b]), k
    print("restatement vs reference, max |log energy difference|:", worst)
    assert worst <= 2e-12


def test_frame_counts_and_every_refusal():
    from dss_amd import _lib, acoustic_vad
    L = _lib.load()
    for n in range(800, 70001):
        assert L.dss_avad_trial_frames_for(n, 800, 160) == (n - 800) // 160 + 1
    for n in (799, 1, 0, -5):
        assert L.dss_avad_trial_frames_for(n, 800, 160) == -1 and b"shorter than one window" in L.dss_last_error()
    assert acoustic_vad.check_trials(100000, [(0, 800), (99200, 800), (99200, 1056)], lead=[0, 0, 256]) == 1 + 1 + 2
    assert acoustic_vad.check_trials(1000, []) == 0

    def refused(n_audio, ranges, lead, message):
        with pytest.raises(_lib.DssError, match=message):
            acoustic_vad.check_trials(n_audio, ranges, lead)
    refused(100000, [(-1, 1000)], 0, "negative first sample or length")
    refused(100000, [(0, -3)], 0, "negative first sample or length")
    refused(100000, [(0, 1000)], -1, "leading zeros")
    refused(100000, [(0, 1000)], 1001, "leading zeros")
    refused(100000, [(0, 1000), (99001, 1000)], 0, "trial 1 .* lies outside the audio")
    refused(100000, [(100001, 1000)], 1000, "lies outside the audio")
    refused(100000, [(0, 1000), (10**12, 1000)], 0, "lies outside the audio")
    refused(100000, [(0, 799)], 0, "shorter than one window")
    first = np.zeros(3, np.int64)
    length = np.full(3, 2**31 - 1, np.int32)
    lead = np.zeros(3, np.int32)
    assert L.dss_avad_check_trials(2**40, 3, first.ctypes.data, length.ctypes.data, lead.ctypes.data, 4, 1) == -1
    assert b"more than 2^31 - 1 frames" in L.dss_last_error()
    assert L.dss_avad_check_trials(1000, 1, None, None, None, 800, 160) == -1 and b"missing array" in L.dss_last_error()
    assert L.dss_avad_check_trials(1000, -1, first.ctypes.data, length.ctypes.data, lead.ctypes.data, 800, 160) == -1
    assert b"negative count" in L.dss_last_error()
    assert L.dss_avad_check_trials(1000, 0, None, None, None, 0, 160) == -1 and b"frame shape" in L.dss_last_error()

    P = acoustic_vad.AvadParams
    good = dict(window=800, shift=160, n_bins=401, n_bands=40, frames_context=5, reserved=0, energy_threshold=4.0,
                energy_mean_scale=1.0, proportion_threshold=0.6)
    assert L.dss_avad_check_params(C.addressof(P(**good))) == 0
    for change, message in ((dict(window=802, n_bins=402), b"multiple of 4"), (dict(shift=0), b"frame shift"), (dict(shift=801), b"frame shift"),
                            (dict(n_bins=400), b"bins"), (dict(n_bands=0), b"mel bands"), (dict(n_bands=65), b"mel bands"),
                            (dict(frames_context=-1), b"frames_context"), (dict(energy_mean_scale=-1.0), b"energy_mean_scale"),
                            (dict(proportion_threshold=1.0), b"proportion_threshold"), (dict(proportion_threshold=0.0), b"proportion_threshold"),
                            (dict(energy_threshold=float("nan")), b"energy_threshold"), (dict(window=2400, shift=480, n_bins=1201), b"does not fit")):
        p = P(**{**good, **change})
        assert L.dss_avad_check_params(C.addressof(p)) == -1 and message in L.dss_last_error(), change
    assert L.dss_avad_check_params(None) == -1
    assert L.dss_avad_create(C.addressof(P(**{**good, "n_bands": 0})), None, None) is None
    # the handle forms refuse a missing handle instead of faulting
    assert L.dss_avad_labels_trials(None, None, 0, 0, None, None, None, None, None, None, None) == -1
    assert L.dss_avad_labels_trials_dev(None, None, 0, 0, None, None, None, None, None, None, None, None) == -1
    assert L.dss_avad_vote_host(None, 0, None, None, None) == -1
    L.dss_avad_destroy(None)


def test_session_arithmetic_by_hand():
    from dss_amd import session
    # prepare_corpus.py:84-87 at 16 kHz / 1 kHz: int(start * 16), int(stop * 16) + 640
    assert session.trial_audio_ranges([(100, 2600), (3000, 3050)], 1000, 16000, 10**6) == [(1600, 40640), (48000, 1440)]
    # a range that ends behind the file is clamped as slicing clamps it; one that starts behind it is empty
    assert session.trial_audio_ranges([(100, 2600), (3000, 3050)], 1000, 16000, 40000) == [(1600, 38400), (40000, 0)]
    # int() truncation at a non-integer ratio: 44100 / 1000 -> int(333 * 44.1) = 14685, int(777 * 44.1) + int(1764.0) = 34265 + 1764
    assert session.trial_audio_ranges([(333, 777)], 1000, 44100, 10**6) == [(14685, 34265 + 1764 - 14685)]
    assert session.trial_audio_ranges([(7, 10)], 3, 16000, None) == [(int(7 * 16000 / 3), int(10 * 16000 / 3) + 640 - int(7 * 16000 / 3))]
    # prepare_corpus.py:118-137: interval = int(stop + 40) - start, windows = floor((interval - 40) / 10); the sign flips on a
    # repeated stimulus and comes back on the next repetition
    stimuli = ["ba", "SILENCE", "du"]
    trials = [(0, 100), (200, 255), (300, 400), (500, 530), (600, 700), (800, 810)]
    labels = ["du", "du", "du", "ba", "SILENCE", "SILENCE"]
    ids = session.trial_ids(trials, labels, stimuli, 1000)
    assert ids.dtype == np.int16
    assert ids.tolist() == [3] * 10 + [-3] * 5 + [3] * 10 + [1] * 3 + [2] * 10 + [-2] * 1
    assert session.trial_ids([], [], stimuli).shape == (0,)
    with pytest.raises(ValueError):
        session.trial_ids([(0, 100)], ["xx"], stimuli)


def test_session_corpus_refuses_misaligned_trials(monkeypatch):
    from dss_amd import session
    calls = []

    def features(recording, trials, fs, bad, contaminated):
        calls.append("features")
        return np.zeros((sum(n // 10 - 4 for _, n in session.trial_ranges(trials, fs)), 128))

    def labels(wav, trials, stimulus_labels, fs, fs_audio, shift_seconds):
        calls.append("labels")
        return np.zeros(sum((n - 800) // 160 + 1 for _, n in session.trial_audio_ranges(trials, fs, fs_audio, len(wav))), dtype=bool)
    monkeypatch.setattr(session, "session_features", features)
    monkeypatch.setattr(session, "session_vad_labels", labels)
    rec = np.zeros((5000, 129))
    stats = np.vstack([np.zeros(128), np.ones(128)])
    trials = [(100, 1100), (2000, 4000)]
    ok = session.session_corpus(rec, np.zeros(16 * 5000, np.int16), trials, ["a", "a"], ["a"], stats)
    assert sorted(ok) == ["hga_activity", "trial_ids", "vad_labels"] and calls == ["features", "labels"]
    assert len(ok["hga_activity"]) == len(ok["vad_labels"]) == len(ok["trial_ids"]) == 100 + 200
    # the wav ends inside the second trial: its labels would be fewer than its feature frames
    with pytest.raises(ValueError, match="trial 1: 200 feature frames but 1[0-9][0-9] label frames"):
        session.session_corpus(rec, np.zeros(16 * 3900, np.int16), trials, ["a", "a"], ["a"], stats)
    assert calls == ["features", "labels"]                                          # refused before anything was launched
    with pytest.raises(ValueError):
        session.session_corpus(rec, np.zeros(16 * 5000, np.int16), trials, ["a", "a"], ["a"], np.zeros((3, 128)))


def test_without_a_device_the_compute_entry_points_say_so():
    from dss_amd import _lib, acoustic_vad
    L = _lib.load()
    if L.dss_device_count() > 0:
        pytest.skip("a HIP device is present")
    P = acoustic_vad.AvadParams(800, 160, 401, 40, 5, 0, 4.0, 1.0, 0.6)
    win = acoustic_vad.hann(800)
    mel = acoustic_vad.mel_filterbank(401, 40, 16000)
    assert L.dss_avad_create(C.addressof(P), win.ctypes.data, mel.ctypes.data) is None
    assert b"no HIP device" in L.dss_last_error()
    with pytest.raises(_lib.DssError):
        acoustic_vad.AcousticVadGPU()
