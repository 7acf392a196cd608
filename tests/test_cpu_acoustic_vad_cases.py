"""The acoustic VAD case table (tests/acoustic_vad_cases.py) without a device: the integers every case is there to reach, as the
package and the library derive them; the refusals just past the limits; the LDS formula on both sides of AVAD_LDS_LIMIT; the
package's window and mel matrix, through the restatement, against what the reference's own EnergyBasedVad gave at every case
(tests/golden/acoustic_vad_cases.npz); and the trial-edge table: its frame counts through dss_avad_check_trials and the
distance of every frame from its trial's threshold."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import acoustic_vad_cases as vc
import acoustic_vad_reference as ref
from dss_amd import _lib, acoustic_vad


def _check(N, shift, bins, bands):
    """dss_avad_check_params at the default vote parameters (the structure is held until the call has returned)."""
    p = acoustic_vad.AvadParams(N, shift, bins, bands, 5, 0, 4.0, 1.0, 0.6)
    return _lib.load().dss_avad_check_params(C.addressof(p))


def test_integers_of_every_case():
    assert len(set(vc.NAMES)) == len(vc.NAMES) == 11
    for c in vc.GEOMETRY:
        assert vc.geometry(c.fs, c.window_length, c.frame_shift) == (c.N, c.shift, c.bins), c.name       # int() truncates a float
        assert c.bins == c.N // 2 + 1 and c.nblk == vc.nblk_of(c.bins) == -(-c.bins // 16)
        mel = acoustic_vad.mel_filterbank(c.bins, c.n_bands, c.fs)
        assert mel.shape == (c.bins, c.n_bands) and int(np.sum(~mel.any(axis=0))) == c.empty, c.name
        assert c.lds == vc.lds_bytes(c.N, c.shift, c.bins, c.n_bands) <= vc.LDS_LIMIT, c.name
        assert acoustic_vad.hann(c.N).shape == (c.N,)
    # the cases sit where their notes say
    by = {c.name: c for c in vc.GEOMETRY}
    assert vc.geometry(*vc.DEFAULT[:3]) == (vc.N0, vc.SHIFT0, 401)
    assert by["no_overlap_64"].shift == by["no_overlap_64"].N and by["no_overlap_64"].nblk == 3 and by["no_overlap_64"].empty == 14
    c = by["shift_1_bands_64"]
    assert c.shift == 1 and c.n_bands == vc.MAX_BANDS and c.empty == 33
    assert vc.TILE * c.n_bands * 8 == 16384 > ((vc.TILE - 1) * c.shift + c.N) * 4 == 380             # the log-mel rows are the larger
    assert vc.TILE * 40 * 8 < ((vc.TILE - 1) * vc.SHIFT0 + vc.N0) * 4                                 # ... at the default the samples are
    assert by["window_4"].N == 4 and by["window_4"].nblk == 1
    assert {c.nblk < 4 for c in vc.GEOMETRY} == {True, False}
    assert vc.TILE * by["bands_8"].n_bands == 256 and vc.TILE * by["bands_9"].n_bands == 256 + vc.TILE and by["bands_1"].n_bands == 1
    # every case's trials: W = 1, 32, 33, 71, inside the case's audio, with samples past the last frame where a shift has room
    for c in vc.GEOMETRY:
        t = vc.trials(c.name)
        assert tuple(ref.frames_of(n, c.N, c.shift) for _, n in t) == vc.TRIAL_FRAMES, c.name
        assert acoustic_vad.check_trials(len(vc.audio(c.name)), t, 0, c.N, c.shift) == sum(vc.TRIAL_FRAMES)
        assert [(n - c.N) % c.shift for _, n in t] == [0, 0, c.shift - 1, min(1, c.shift - 1)], c.name


def test_check_params_accepts_the_cases_and_refuses_their_successors():
    L = _lib.load()
    for c in vc.GEOMETRY:
        assert _check(c.N, c.shift, c.bins, c.n_bands) == 0, (c.name, L.dss_last_error())
    assert [r.name for r in vc.REFUSALS] == ["window_924", "shift_313", "fs_22050", "bands_65"]
    for r in vc.REFUSALS:
        N, shift, bins = vc.geometry(r.fs, r.window_length, r.frame_shift)
        assert (N, shift) == (r.N, r.shift), r.name
        assert _check(N, shift, bins, r.n_bands) == -1, r.name
        assert r.message.encode() in L.dss_last_error(), (r.name, L.dss_last_error())
        if r.lds is not None:
            assert vc.lds_bytes(N, shift, bins, r.n_bands) == r.lds > vc.LDS_LIMIT, r.name
        with pytest.raises(_lib.DssError, match=r.message):           # the constructor refuses before it asks for a device
            acoustic_vad.AcousticVadGPU(fs=r.fs, window_length=r.window_length, frame_shift=r.frame_shift, n_bands=r.n_bands)


def test_lds_formula_on_both_sides_of_the_limit():
    def accepted(N, shift, bands=40):
        return _check(N, shift, N // 2 + 1, bands) == 0
    assert vc.lds_bytes(920, 160, 461, 40) == 163616 <= vc.LDS_LIMIT < vc.lds_bytes(924, 160, 463, 40) == 164240
    assert vc.lds_bytes(800, 312, 401, 40) == 163744 <= vc.LDS_LIMIT < vc.lds_bytes(800, 313, 401, 40) == 163872
    assert vc.lds_bytes(800, 160, 401, 40) == (3 * 800 + 32 * 401) * 8 + 5760 * 4          # the default, by hand
    assert vc.lds_bytes(64, 1, 33, 64) == (3 * 64 + 32 * 33) * 8 + 16384                   # the log-mel arm, by hand
    assert vc.lds_bytes(4, 1, 3, 1) == (12 + 96) * 8 + 256 and vc.lds_bytes(4, 2, 3, 1) == (12 + 96) * 8 + 272    # 264 rounded up to 16
    # the library flips exactly where the restated formula passes the limit: along the window at a shift of 160, along the
    # shift under a window of 800, and along both with 64 bands
    for N in range(4, 1400, 4):
        assert accepted(N, 160 if N >= 160 else N) == (vc.lds_bytes(N, min(N, 160), N // 2 + 1, 40) <= vc.LDS_LIMIT), N
    for shift in range(1, 801):
        assert accepted(800, shift) == (vc.lds_bytes(800, shift, 401, 40) <= vc.LDS_LIMIT), shift
        assert accepted(800, shift, 64) == (vc.lds_bytes(800, shift, 401, 64) <= vc.LDS_LIMIT), shift
    assert accepted(920, 160) and not accepted(924, 160) and accepted(800, 312) and not accepted(800, 313)


@pytest.fixture(scope="module")
def cases_fixture(golden):
    g = golden("acoustic_vad_cases.npz")
    assert tuple(str(n) for n in g["names"]) == vc.NAMES
    return g


def test_fixture_is_the_tables(cases_fixture):
    g = cases_fixture
    prov = str(g["provenance"])
    assert "reference classes" in prov and "h5py placeholder untouched" in prov and "hanning" in prov and "MelFilterBank" in prov
    assert g["geometry"].tolist() == [[c.fs, c.N, c.shift, c.bins, c.n_bands] for c in vc.GEOMETRY]
    assert g["band_wrapper"].tolist() == [c.n_bands != 40 for c in vc.GEOMETRY]
    assert g["trials"].tolist() == [list(t) for c in vc.GEOMETRY for t in vc.trials(c.name)]
    assert g["frame_counts"].tolist() == list(vc.TRIAL_FRAMES) * len(vc.GEOMETRY)
    n = int(g["frame_counts"].sum())
    assert g["log_energy"].shape == g["labels"].shape == (n,) and g["thresholds"].shape == (4 * len(vc.GEOMETRY),)
    assert g["log_energy"].dtype == np.float64 and g["labels"].dtype == bool
    assert g["labels"].any() and not g["labels"].all()
    for k, c in enumerate(vc.GEOMETRY):
        wav = vc.audio(c.name)
        assert g["audio_seed"][k].tolist() == [vc.audio_seed(c.name), len(wav)]
        assert hashlib.sha256(wav.tobytes()).digest() == g["audio_sha"][k].tobytes(), c.name
    # no stored frame lies within GAP of its trial's threshold: labels are comparable on every frame, nothing is left out
    b = np.concatenate([[0], np.cumsum(g["frame_counts"])])
    for k in range(len(g["thresholds"])):
        assert np.min(np.abs(g["log_energy"][b[k]:b[k + 1]] - g["thresholds"][k])) >= vc.GAP, k


def test_bounds_come_from_the_cpu_and_stay_under_the_cap(cases_fixture):
    g = cases_fixture
    b = np.concatenate([[0], np.cumsum(g["frame_counts"])])
    for k, c in enumerate(vc.GEOMETRY):
        le = g["log_energy"][b[4 * k]:b[4 * k + 4]]
        assert vc.U[c.name] == vc.ulp_of_largest(le), c.name
        assert vc.bound(c.name) == vc.MARGIN * max(c.D, vc.U[c.name]) and 0 < vc.bound(c.name) <= vc.CAP, c.name
        assert vc.GAP >= 1e4 * vc.bound(c.name)
    import test_gpu_acoustic_vad
    assert vc.LOG_ENERGY_BOUND == test_gpu_acoustic_vad.LOG_ENERGY_BOUND <= vc.CAP and vc.GAP == test_gpu_acoustic_vad.GAP


@pytest.mark.parametrize("name", vc.NAMES)
def test_tables_reproduce_the_reference_at_every_case(cases_fixture, name):
    """The fixture holds no matrices.  The restatement, fed the package's mel_filterbank and hann, stays within 1.5 D of the
    reference's energies and gives its labels on every frame: a band edge off by one bin, a wrong
    normalisation or a periodic window would each move the energies by far more."""
    g, c, k = cases_fixture, vc.case(name), vc.NAMES.index(name)
    b = np.concatenate([[0], np.cumsum(g["frame_counts"])])
    win, mel = acoustic_vad.hann(c.N), acoustic_vad.mel_filterbank(c.bins, c.n_bands, c.fs)
    wav = vc.audio(name)
    worst = 0.0
    for j, (first, n) in enumerate(vc.trials(name)):
        a, z = b[4 * k + j], b[4 * k + j + 1]
        le = ref.log_energy(ref.trial_samples(wav, first, n, 0), win, mel, shift=c.shift)
        assert le.shape == (z - a,)
        worst = max(worst, float(np.max(np.abs(le - g["log_energy"][a:z]))))
        labels, _, gap = ref.vote(le)
        assert gap >= vc.GAP
        assert np.array_equal(labels, g["labels"][a:z]), (name, j)
        host, host_thr = acoustic_vad.vote_host(g["log_energy"][a:z])
        assert np.array_equal(host, g["labels"][a:z]) and abs(host_thr - g["thresholds"][4 * k + j]) <= 1e-12 * abs(host_thr), (name, j)
    print(f"{name}: restatement vs reference, max |log energy difference| {worst:.3e}, D {c.D:.3e}")
    assert worst <= 1.5 * c.D


def test_edge_table_frame_counts():
    assert len(set(vc.EDGE_NAMES)) == len(vc.EDGE_NAMES)
    for which in ("speech", "noise"):
        n_audio = len(vc.edge_audio(which))
        for e in vc.edges(which):
            assert acoustic_vad.check_trials(n_audio, [(e.first, e.length)], e.lead) == e.W == ref.frames_of(e.length), e.name
            assert acoustic_vad.trial_frames(e.length) == e.W
        es = vc.edges(which)
        assert acoustic_vad.check_trials(n_audio, [(e.first, e.length) for e in es], [e.lead for e in es]) == sum(e.W for e in es)
    by = {e.name: e for e in vc.EDGES}
    n_audio = len(vc.edge_audio("speech"))
    assert {by[k].W for k in ("w_31", "w_32", "w_33", "w_64", "w_65")} == {31, 32, 33, 64, 65}
    assert (by["past_159"].length - vc.N0) % vc.SHIFT0 == 159
    assert {e.lead for e in vc.EDGES} >= {0, 1, 159, 160, 161, 800, 32 * 160 + 7, vc.TILE_SPAN + 7} and vc.TILE_SPAN == 5760
    assert by["lead_5127"].W > vc.TILE and by["lead_tile_span"].W > vc.TILE
    assert by["lead_whole"].lead == by["lead_whole"].length and by["lead_whole_at_end"].first == n_audio
    assert by["from_sample_0"].first == 0
    for k in ("to_last_sample", "to_last_sample_led"):
        assert by[k].first + by[k].length - by[k].lead == n_audio
    assert (by["twice_a"].first, by["twice_a"].length) == (by["twice_b"].first, by["twice_b"].length) and by["twice_a"].lead != by["twice_b"].lead
    noise = vc.edge_audio("noise")
    assert noise.min() == -32768 and noise.max() == 32767 and by["full_scale_noise"].length == len(noise)
    # one past either end of the audio is refused
    e = by["to_last_sample"]
    with pytest.raises(_lib.DssError, match="lies outside the audio"):
        acoustic_vad.check_trials(n_audio, [(e.first + 1, e.length)], e.lead)
    with pytest.raises(_lib.DssError, match="lies outside the audio"):
        acoustic_vad.check_trials(n_audio, [(n_audio + 1, 800)], 800)
    # the vote's list and the invariance leads
    assert [ref.frames_of(n) for _, n in vc.vote_trials()] == list(vc.VOTE_FRAMES)
    assert acoustic_vad.check_trials(vc.VOTE_AUDIO_SAMPLES, vc.vote_trials()) == sum(vc.VOTE_FRAMES)
    assert vc.invariance_leads(800, 160) == (1, 159, 160, 161, 800, 5767) and vc.invariance_leads(64, 1) == (1, 2, 64, 102)


def test_no_edge_frame_is_near_its_threshold():
    """On the restatement alone: every frame of every edge trial, and of the vote's list at the threshold parameters of the GPU
    test, is farther than GAP from its trial's threshold, so labels are compared on every frame."""
    win, mel = acoustic_vad.hann(vc.N0), acoustic_vad.mel_filterbank(401, 40, 16000)
    frames = 0
    for e in vc.EDGES:
        le = ref.log_energy(ref.trial_samples(vc.edge_audio(e.audio), e.first, e.length, e.lead), win, mel)
        _, thr, gap = ref.vote(le)
        assert len(le) == e.W and gap >= vc.GAP, (e.name, gap)
        frames += e.W
        if e.lead == e.length:
            assert np.all(le == le[0]) and abs(le[0] - 80 * np.log(1e-7)) < 1e-9
    assert frames == sum(e.W for e in vc.EDGES) == 515
