"""Acoustic VAD labels over a trial list on the GPU (dss_avad_labels_trials*), held to tests/golden/acoustic_vad.npz, which the
reference's own EnergyBasedVad produced (tools/make_golden_acoustic_vad.py), and beyond the fixture to the float64 numpy
restatement in tests/acoustic_vad_reference.py.

Labels: equal to the reference's on EVERY fixture frame (no frame of the fixture lies within 0.8 of its trial's threshold).
Log energy: the reference's arithmetic is numpy's pocketfft and BLAS, the kernel's a table DFT on the fp64 MFMA with OCML's
log, so they agree to rounding, not bit for bit.  Measured on an MI355X over the 1376 fixture frames (values between -1290
and -148): the kernel's worst deviation from the fixture is 6.82e-13; the numpy restatement's is 7.96e-13.  The
bound is 4x the larger of the two, 3.18e-12, and must stay under the cap 1e-10, which is still 10^9 times below the smallest gap.
"""
import hashlib

import numpy as np
import pytest

import acoustic_vad_reference as ref
from dss_amd.synthetic import synthetic_ecog, synthetic_speech_audio

pytestmark = pytest.mark.gpu

MEASURED_KERNEL = 6.83e-13          # max |log energy - fixture| of avad_energy_kernel on an MI355X
MEASURED_RESTATEMENT = 7.96e-13     # the same figure of tests/acoustic_vad_reference.py (numpy, direct DFT)
LOG_ENERGY_BOUND = 4 * max(MEASURED_KERNEL, MEASURED_RESTATEMENT)
GAP = 1e-6                          # beyond the fixture: frames whose vote sees an energy this close to the threshold are left out
LEFT_OUT_CAP = 0.001                # ... and may be at most 0.1 % of a case


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("acoustic_vad.npz")
    seed, n, fs, z0, z1 = (int(v) for v in g["audio_seed"])
    wav = synthetic_speech_audio(seed, n, fs)
    wav[z0:z1] = 0
    assert hashlib.sha256(wav.tobytes()).digest() == g["audio_sha"].tobytes()
    t = g["trials"]
    return {"g": g, "wav": wav, "ranges": [(int(a), int(b)) for a, b in t[:, :2]], "lead": [int(v) for v in t[:, 2]],
            "silence": [bool(v) for v in t[:, 3]], "bounds": np.concatenate([[0], np.cumsum(g["frame_counts"])])}


@pytest.fixture(scope="module")
def vad():
    from dss_amd.acoustic_vad import AcousticVadGPU
    v = AcousticVadGPU()
    yield v
    v.close()


def _against_restatement(v, wav, ranges, lead, silence=None, **params):
    """One call over the list against the restatement trial by trial; returns (frames, frames left out)."""
    labels, le, thr = v.labels_trials(wav, ranges, lead=lead, silence=silence, return_energy=True)
    ctx = params.get("frames_context", 5)
    pos = total = left_out = 0
    for k, (first, n) in enumerate(ranges):
        want_le = ref.log_energy(ref.trial_samples(wav, first, n, lead), v.window_fn, v.mel)
        W = len(want_le)
        assert np.max(np.abs(le[pos:pos + W] - want_le)) <= LOG_ENERGY_BOUND, k
        want, want_thr, _ = ref.vote(want_le, **params)
        assert abs(thr[k] - want_thr) <= LOG_ENERGY_BOUND + 1e-12 * abs(want_thr), k
        if silence is not None and silence[k]:
            want[:] = False
        skip = ref.near_threshold(want_le, want_thr, ctx, GAP)
        assert np.array_equal(labels[pos:pos + W][~skip], want[~skip]), k
        pos, total, left_out = pos + W, total + W, left_out + int(skip.sum())
    assert pos == len(labels)
    return total, left_out


def test_fixture_in_one_call(fx, vad):
    g = fx["g"]
    labels, le, thr = vad.labels_trials(fx["wav"], fx["ranges"], lead=fx["lead"], silence=fx["silence"], return_energy=True)
    assert labels.dtype == bool and labels.shape == g["labels"].shape
    assert np.array_equal(labels, g["labels"])                                      # every frame, none left out
    worst = float(np.max(np.abs(le - g["log_energy"])))
    print("kernel vs reference, max |log energy difference|:", worst, "bound", LOG_ENERGY_BOUND)
    assert LOG_ENERGY_BOUND <= 1e-10
    assert worst <= LOG_ENERGY_BOUND
    assert np.max(np.abs(thr - g["thresholds"])) <= LOG_ENERGY_BOUND
    # the plain form returns the same labels
    assert np.array_equal(vad.labels_trials(fx["wav"], fx["ranges"], lead=fx["lead"], silence=fx["silence"]), g["labels"])


def test_list_equals_trial_by_trial_in_any_order(fx, vad):
    wav, b = fx["wav"], fx["bounds"]
    one = vad.labels_trials(wav, fx["ranges"], lead=fx["lead"], silence=fx["silence"], return_energy=True)
    again = vad.labels_trials(wav, fx["ranges"], lead=fx["lead"], silence=fx["silence"], return_energy=True)
    assert all(np.array_equal(x, y) for x, y in zip(one, again))                    # fixed-order sums: run to run bit for bit
    for k in range(len(fx["ranges"])):
        lab, le, thr = vad.labels_trials(wav, [fx["ranges"][k]], lead=fx["lead"][k], silence=[fx["silence"][k]], return_energy=True)
        assert np.array_equal(lab, one[0][b[k]:b[k + 1]]) and np.array_equal(le, one[1][b[k]:b[k + 1]]), k
        assert thr[0] == one[2][k], k
    perm = np.random.default_rng(11).permutation(len(fx["ranges"]))
    assert not np.array_equal(perm, np.arange(len(perm)))
    lab, le, thr = vad.labels_trials(wav, [fx["ranges"][k] for k in perm], lead=[fx["lead"][k] for k in perm],
                                     silence=[fx["silence"][k] for k in perm], return_energy=True)
    pos = 0
    for k in perm:                                                                  # output in LIST order, not longest first
        W = b[k + 1] - b[k]
        assert np.array_equal(lab[pos:pos + W], one[0][b[k]:b[k + 1]]) and np.array_equal(le[pos:pos + W], one[1][b[k]:b[k + 1]]), k
        pos += W
    assert np.array_equal(thr, one[2][perm])


def test_device_resident_form_equals_the_host_form(fx, vad):
    import torch
    host = vad.labels_trials(fx["wav"], fx["ranges"], lead=fx["lead"], silence=fx["silence"], return_energy=True)
    d_wav = torch.from_numpy(fx["wav"]).cuda()
    lab, le, thr = vad.labels_trials_torch(d_wav, fx["ranges"], lead=fx["lead"], silence=fx["silence"], return_energy=True)
    torch.cuda.synchronize()
    assert lab.dtype == torch.uint8 and np.array_equal(lab.cpu().numpy().astype(bool), host[0])
    assert np.array_equal(le.cpu().numpy(), host[1]) and np.array_equal(thr.cpu().numpy(), host[2])
    only = vad.labels_trials_torch(d_wav, fx["ranges"], lead=fx["lead"], silence=fx["silence"])
    torch.cuda.synchronize()
    assert np.array_equal(only.cpu().numpy().astype(bool), host[0])
    # on a stream of its own, behind work already queued there
    s = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(8):
            a = a @ a * 1e-3
        staged = d_wav.clone()                                                      # the audio itself arrives on that stream
        lab, le, thr = vad.labels_trials_torch(staged, fx["ranges"], lead=fx["lead"], silence=fx["silence"], return_energy=True)
    s.synchronize()
    assert np.array_equal(lab.cpu().numpy().astype(bool), host[0]) and np.array_equal(le.cpu().numpy(), host[1])
    assert np.array_equal(thr.cpu().numpy(), host[2])


def _session_trials(seed, n_audio, n_trials, fs=16000):
    rng = np.random.default_rng(seed)
    ranges = []
    for _ in range(n_trials):
        n = int(rng.uniform(1.0, 4.0) * fs) + 640
        ranges.append((int(rng.integers(0, n_audio - n)), n))
    return ranges


def test_a_ten_minute_session_against_the_restatement(vad):
    n_audio = 600 * 16000
    wav = synthetic_speech_audio(8200, n_audio)
    ranges = _session_trials(8201, n_audio, 300)
    silence = [k % 17 == 3 for k in range(300)]
    total, left_out = _against_restatement(vad, wav, ranges, 256, silence)
    print("ten-minute session:", total, "frames,", left_out, "left out")
    assert total > 60000 and left_out <= LEFT_OUT_CAP * total


def test_a_sixty_second_trial(vad):
    wav = synthetic_speech_audio(8300, 70 * 16000)
    total, left_out = _against_restatement(vad, wav, [(32000, 60 * 16000 + 640), (5000, 800)], 256)
    assert total == 6000 + 1 and left_out <= LEFT_OUT_CAP * total


@pytest.mark.parametrize("params", [dict(frames_context=0), dict(frames_context=8), dict(proportion_threshold=0.3),
                                    dict(energy_mean_scale=0.0), dict(energy_threshold=-2.0),
                                    dict(energy_mean_scale=0.0, energy_threshold=-400.0)])
def test_other_parameters(params):
    from dss_amd.acoustic_vad import AcousticVadGPU
    n_audio = 60 * 16000
    wav = synthetic_speech_audio(8400, n_audio)
    ranges = _session_trials(8401, n_audio, 24)
    v = AcousticVadGPU(**params)
    try:
        total, left_out = _against_restatement(v, wav, ranges, 256, None, **params)
    finally:
        v.close()
    assert left_out <= LEFT_OUT_CAP * total


def test_refusals_reach_the_caller(vad):
    from dss_amd import _lib
    wav = np.zeros(20000, np.int16)
    with pytest.raises(_lib.DssError, match="shorter than one window"):
        vad.labels_trials(wav, [(0, 799)])
    with pytest.raises(_lib.DssError, match="lies outside the audio"):
        vad.labels_trials(wav, [(19500, 1000)])
    with pytest.raises(ValueError):
        vad.labels_trials(wav.astype(np.float64), [(0, 1000)])
    assert vad.labels_trials(wav, []).shape == (0,)
    lab, le, thr = vad.labels_trials(wav, [(100, 1600)], lead=1600, return_energy=True)    # nothing but leading zeros
    assert not lab.any() and np.all(le == le[0]) and abs(le[0] - 80 * np.log(1e-7)) < 1e-9


def test_session_corpus(golden):
    from dss_amd import session
    g = golden("session.npz")
    seed, T, c_raw = (int(v) for v in g["recording_seed"])
    rec = synthetic_ecog(seed, T, c_raw)
    fs = int(g["fs"][0])
    trials = [tuple(int(v) for v in t) for t in g["trials"]][1:]                     # the first (45 rows) is shorter than one audio window
    labels = ["ba", "ba", "SILENCE", "du", "du"]
    stimuli = ["SILENCE", "ba", "du"]
    wav = synthetic_speech_audio(8500, 16 * T)
    stats = session.normalization_statistics(rec, trials, fs)
    corpus = session.session_corpus(rec, wav, trials, labels, stimuli, stats, fs=fs)
    assert sorted(corpus) == ["hga_activity", "trial_ids", "vad_labels"]
    feats = session.session_features(rec, trials, fs)
    assert corpus["hga_activity"].dtype == np.float64 and np.array_equal(corpus["hga_activity"], (feats - stats[0]) / stats[1])
    assert corpus["vad_labels"].dtype == bool and corpus["trial_ids"].dtype == np.int16
    assert len(corpus["hga_activity"]) == len(corpus["vad_labels"]) == len(corpus["trial_ids"]) == int(g["frame_counts"][1:].sum())
    counts = g["frame_counts"][1:]
    assert corpus["trial_ids"].tolist() == sum(([c] * int(w) for c, w in zip((2, -2, 1, 3, -3), counts)), [])
    b = np.concatenate([[0], np.cumsum(counts)])
    assert not corpus["vad_labels"][b[2]:b[3]].any()                                # the SILENCE trial
    want = session.session_vad_labels(wav, trials, labels, fs)
    assert np.array_equal(corpus["vad_labels"], want)
    with pytest.raises(_lib_error()):
        session.session_corpus(rec, wav, [tuple(int(v) for v in g["trials"][0])], ["ba"], stimuli, stats, fs=fs)


def _lib_error():
    from dss_amd import _lib
    return _lib.DssError
