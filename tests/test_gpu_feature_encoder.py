"""The LPC feature encoder's kernels (Part 16, csrc/feature_encoder.hip) against the float64 definition in
tests/feature_encoder_reference.py, on the case table of tests/feature_encoder_cases.py.

Outputs 0..17: the reference is fp64 and the kernel is fp64 rounded to float32 once, so they are within one float32 ulp (at the
value) of the float32-rounded reference; derived, not measured.  Outputs 20..35: the decoder's own chain on the call's own
float32 cepstrum, bit for bit the checker's lpc_from_cepstrum.  Scores: against the reference's scores recomputed from the
call's own float32 LPC taps, so that one-ulp cepstrum differences do not enter.  Measured on an MI355X over the whole case
table: the largest |kernel - reference| is MEASURED_SCORES = 2.331e-15 (the full-scale square wave; 7.8e-16 elsewhere); the
bound is four times that, 9.324e-15, and stays below 1e-9 (the quantities
are O(1) fp64 sums of 80 terms).  Output 18: exact in every frame of every case (the case table's decision margins are at least
1e-9, tests/test_cpu_feature_encoder.py).  Output 19: one float32 ulp + 1e-6.
"""
import numpy as np
import pytest

import feature_encoder_cases as K
import feature_encoder_reference as R

pytestmark = pytest.mark.gpu

MEASURED_SCORES = 2.331e-15        # max |score - reference| on an MI355X over the case table (the full-scale square wave)
SCORE_BOUND = 4 * MEASURED_SCORES
assert SCORE_BOUND <= 1e-9

CASES = K.cases()


@pytest.fixture(scope="module")
def lpc_fn(oracle):
    from dss_amd.lpcnet_weights import synthetic_blob
    m = oracle.lpcnet_model(synthetic_blob(0))
    return lambda cep: oracle.lpc_from_cepstrum(m, np.ascontiguousarray(cep, dtype=np.float32))


@pytest.fixture(scope="module")
def enc():
    from dss_amd.feature_encoder import LpcFeatureEncoderGPU
    e = LpcFeatureEncoderGPU()
    yield e
    e.close()


@pytest.fixture(scope="module")
def runs(enc, lpc_fn):
    """Every case once: the kernel's 36 outputs and score tap, and the reference (its own cepstrum; residual, scores and track
    from the call's float32 cepstrum and taps)."""
    out = {}
    for name, trials in CASES:
        audio, offs = K.concatenate(trials)
        got, fo = enc.features_trials(audio, offs, total=True)
        scores = enc.scores()
        own, fo_ref = R.encode_trials(audio, offs, lpc_fn)
        fed, _ = R.encode_trials(audio, offs, lpc_fn, cepstrum32=got[:, :18], lpc=got[:, 20:])
        assert fo.tolist() == fo_ref.tolist()
        out[name] = dict(audio=audio, offs=offs, got=got, fo=fo, scores=scores, own=own, fed=fed)
    return out


def _ulp32(v):
    return np.spacing(np.abs(v.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_case(runs, lpc_fn, name):
    r = runs[name]
    got, fo = r["got"], r["fo"]
    assert got.dtype == np.float32 and got.shape == (fo[-1], 36) and np.isfinite(got).all()
    worst_scores = 0.0
    for k, (own, fed) in enumerate(zip(r["own"], r["fed"])):
        g = got[fo[k]:fo[k + 1]]
        F = len(g)
        assert F == (r["offs"][k + 1] - r["offs"][k]) // 160
        if not F:
            continue
        # outputs 0..17: one float32 ulp of the float32-rounded fp64 reference
        want = own.cepstrum64.astype(np.float32)
        err = np.abs(g[:, :18].astype(np.float64) - want.astype(np.float64))
        print(f"{name}[{k}] cepstrum: worst error {float((err / _ulp32(want)).max()):.2f} ulp")
        assert (err <= _ulp32(want)).all(), (name, k)
        # outputs 20..35: the decoder's chain on the call's own cepstrum, bit for bit
        lpc = np.stack([lpc_fn(g[i, :18]) for i in range(F)])
        assert np.array_equal(g[:, 20:], lpc), (name, k)
        # scores: the tap against the reference's, from the call's own taps
        s = r["scores"][2 * fo[k]:2 * fo[k + 1]]
        d = float(np.abs(s - fed.scores).max())
        worst_scores = max(worst_scores, d)
        print(f"{name}[{k}] scores: max |kernel - reference| {d:.3e}, reference margin {fed.margin:.1e}")
        assert d <= SCORE_BOUND, (name, k, d)
        assert fed.margin >= K.MIN_MARGIN
        # output 18: exact; output 19: one ulp + 1e-6
        assert np.array_equal(g[:, 18], fed.features[:, 18]), (name, k, g[:, 18], fed.features[:, 18])
        e19 = np.abs(g[:, 19].astype(np.float64) - fed.features[:, 19].astype(np.float64))
        assert (e19 <= _ulp32(fed.features[:, 19]) + 1e-6).all(), (name, k)
    print(f"{name}: worst score error {worst_scores:.3e}")


def test_all_zero_trial_is_exact(runs):
    r = runs["signals"]
    k = 3
    g = r["got"][r["fo"][k]:r["fo"][k + 1]]
    own = r["own"][k]
    assert np.array_equal(g[:, :20], own.features[:, :20])        # cepstrum included: equal inputs, equal order, equal bits
    assert np.array_equal(g[:, 20:], own.features[:, 20:])
    assert not r["scores"][2 * r["fo"][k]:2 * r["fo"][k + 1]].any()


def test_host_and_device_entry_points_give_the_same_bits(enc, runs):
    import torch
    for name in ("lengths", "tile_edges", "empty_between"):
        r = runs[name]
        d_audio = torch.from_numpy(r["audio"]).cuda()
        out, fo = enc.features_trials_torch(d_audio, r["offs"], total=True)
        assert out.is_cuda and out.dtype == torch.float32 and fo.tolist() == r["fo"].tolist()
        assert np.array_equal(out.cpu().numpy(), r["got"])
        assert np.array_equal(enc.scores(), r["scores"])
        out20, _ = enc.features_trials_torch(d_audio, r["offs"])
        assert out20.shape == (fo[-1], 20) and np.array_equal(out20.cpu().numpy(), r["got"][:, :20])


def test_a_trial_alone_equals_the_trial_in_a_list(enc, runs):
    name, trials = CASES[2]
    r = runs[name]
    for k in (0, 2, 5):
        alone = enc.compute_LPC_features(trials[k])
        assert alone.dtype == np.float32 and np.array_equal(alone, r["got"][r["fo"][k]:r["fo"][k + 1], :20])


def test_wrapper_checks_and_refusals(enc):
    from dss_amd import _lib, feature_encoder
    with pytest.raises(TypeError):
        enc.compute_LPC_features([0] * 160)
    with pytest.raises(ValueError, match="wrong number of dimensions"):
        enc.compute_LPC_features(np.zeros((2, 160), np.int16))
    with pytest.raises(ValueError, match="dtype mismatch"):
        enc.compute_LPC_features(np.zeros(160, np.float32))
    assert enc.compute_LPC_features(np.zeros(159, np.int16)).shape == (0, 20)
    audio = K.white(1000, 70)
    out, fo = enc.features_trials(audio, [0])                      # an empty list is a no-op
    assert out.shape == (0, 20) and fo.tolist() == [0] and enc.scores().shape == (0, 256)
    with pytest.raises(_lib.DssError, match="before its start"):
        enc.features_trials(audio, [0, 500, 400])
    with pytest.raises(_lib.DssError, match="behind the audio"):
        enc.features_trials(audio, [0, 500, 1001])
    with pytest.raises(_lib.DssError, match="negative"):
        enc.features_trials(audio, [-1, 500])
    assert feature_encoder.frame_offsets([0, 159, 160, 480, 480]).tolist() == [0, 0, 0, 2, 2]
    again, _ = enc.features_trials(audio, [0, 1000])               # the handle is as good as before
    assert again.shape == (6, 20) and np.isfinite(again).all()


def test_session_corpus_with_lpc_coefficients(golden, enc):
    from dss_amd import session
    from dss_amd.synthetic import synthetic_ecog, synthetic_speech_audio
    g = golden("session.npz")
    seed, T, c_raw = (int(v) for v in g["recording_seed"])
    rec = synthetic_ecog(seed, T, c_raw)
    fs = int(g["fs"][0])
    trials = [tuple(int(v) for v in t) for t in g["trials"]][1:]    # the first (45 rows) is shorter than one audio window
    labels = ["ba", "ba", "SILENCE", "du", "du"]
    stimuli = ["SILENCE", "ba", "du"]
    wav = synthetic_speech_audio(8500, 16 * T)
    stats = session.normalization_statistics(rec, trials, fs)
    plain = session.session_corpus(rec, wav, trials, labels, stimuli, stats, fs=fs)
    assert sorted(plain) == ["hga_activity", "trial_ids", "vad_labels"]
    corpus = session.session_corpus(rec, wav, trials, labels, stimuli, stats, fs=fs, lpc_coefficients=True)
    assert sorted(corpus) == ["hga_activity", "lpc_coefficients", "trial_ids", "vad_labels"]
    for key in plain:
        assert np.array_equal(plain[key], corpus[key])
    lpc = corpus["lpc_coefficients"]
    assert lpc.dtype == np.float32 and lpc.shape == (len(corpus["hga_activity"]), 20)
    audio, offs = session.session_trial_audio(wav, trials, labels, fs)
    counts = g["frame_counts"][1:]
    b = np.concatenate([[0], np.cumsum(counts)])
    for k in range(len(trials)):
        feats = enc.compute_LPC_features(np.ascontiguousarray(audio[offs[k]:offs[k + 1]]))
        assert np.array_equal(lpc[b[k]:b[k + 1]], feats[3:-1]), k
    assert np.array_equal(lpc, session.session_lpc_coefficients(wav, trials, labels, fs))
    # the wav ends inside the last trial: its rows would be fewer than its feature frames
    with pytest.raises(ValueError, match="trial 4"):
        session.session_corpus(rec, wav[:16 * 2900], trials, labels, stimuli, stats, fs=fs, lpc_coefficients=True)
