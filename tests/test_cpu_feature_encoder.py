"""The LPC feature encoder's definition (tests/feature_encoder_reference.py) pinned part by part against numpy / scipy / closed
forms, and the case table's decision margins.  Parity with xiph's encoder is NOT pinned (no copy of it is at hand); what is
pinned is that the statement is what it says.  No GPU needed.

Pitch on pulse trains, as run: periods 33, 34 and 100 lock from the fourth frame on (in fact from the second) with f19 > 0, for
each of the three seeds.  Periods 255 and 256 do NOT lock: a sub-frame is 80 samples, so two out of three sub-frames hold no
pulse, their scores are noise and the track leaves the lag in some frames (255 reads 253..255, 256 mostly reads 255).  Every
period from 100 to 167 locks, above that only scattered ones, 213 the largest; 167 and 213 are tested in their place.
"""
import numpy as np
import pytest

import feature_encoder_cases as K
import feature_encoder_reference as R


@pytest.fixture(scope="module")
def lpc_fn(oracle):
    from dss_amd.lpcnet_weights import synthetic_blob
    m = oracle.lpcnet_model(synthetic_blob(0))          # the chain's tables are derived, not the model's
    return lambda cep: oracle.lpc_from_cepstrum(m, np.ascontiguousarray(cep, dtype=np.float32))


@pytest.fixture(scope="module")
def encoded(lpc_fn):
    """Every case of the table through the reference, once."""
    return {name: R.encode_trials(*K.concatenate(trials), lpc_fn) for name, trials in K.cases()}


def test_window_and_spectrum():
    k = np.arange(160) + .5
    half = np.sin(.5 * np.pi * np.sin(.5 * np.pi * k / 160) ** 2)
    w = R.window_table()
    assert w.dtype == np.float32 and np.array_equal(w, np.concatenate([half, half[::-1]]).astype(np.float32))
    assert np.allclose(w[:160].astype(np.float64) ** 2 + w[160:].astype(np.float64) ** 2, 1.0, atol=1e-6)   # power complementary
    x = R.preemphasis(K.white(160 * 5, 40))
    xw = R.windowed_frames(x, 5)
    assert np.array_equal(xw[0, :160], np.zeros(160)) and np.array_equal(xw[1, :160], x[:160] * w[:160].astype(np.float64))
    X = R.spectrum(xw)
    want = np.fft.rfft(xw, axis=1) / 320
    assert X.shape == (5, 161) and np.abs(X - want).max() <= 1e-12 * np.abs(want).max()


def test_preemphasis():
    s = np.array([100, -200, 300], np.int16)
    c = float(np.float32(0.85))
    assert np.array_equal(R.preemphasis(s), [100.0, -200 - c * 100, 300 + c * 200])


def test_dct_equals_scipy_and_round_trips_through_the_decoders_inverse():
    from scipy.fft import dct as scipy_dct
    rng = np.random.default_rng(41)
    Ly = rng.uniform(-2, 6, (7, 18))
    i, j = np.arange(18.0)[:, None], np.arange(18.0)[None, :]
    D64 = np.cos((i + .5) * j * np.pi / 18)
    D64[:, 0] *= np.sqrt(.5)
    assert np.array_equal(R.dct_table(), D64.astype(np.float32))
    want = scipy_dct(Ly, type=2, norm="ortho", axis=1)
    assert np.abs(R.dct(Ly, D64) - want).max() < 1e-13
    # the float32 table moves every term by at most 2^-24 relative: 18 terms of at most 6
    assert np.abs(R.dct(Ly) - want).max() < 18 * 6 * 2.0 ** -24 * np.sqrt(2 / 18)

    def inverse(c, D):      # lpcnet_frame.hip / lpc_chain.h: tmp = c, tmp[0] += 4, Ex[i] = sqrt(2/18) sum_j tmp[j] D[i][j]
        tmp = c.copy()
        tmp[:, 0] += 4
        return (tmp @ D.T) * np.sqrt(2. / 18)
    c = R.dct(Ly, D64)
    c[:, 0] -= 4
    assert np.abs(inverse(c, D64) - Ly).max() < 1e-12           # the transform pair, scalings and the offset of 4
    c32 = R.dct(Ly)
    c32[:, 0] -= 4
    # with the float32 table on both sides the pair is orthogonal to the table's rounding only: 2 x 18 terms of at most 6 x 2^-24
    assert np.abs(inverse(c32, R.dct_table().astype(np.float64)) - Ly).max() < 2 * 18 * 6 * 2.0 ** -24


def test_band_weights_are_a_partition():
    w = R.band_weights()
    assert w.shape == (18, 161) and (w >= 0).all()
    assert np.abs(w.sum(axis=0) - 1).max() < 1e-15              # every bin 0..160, before the two edge doublings
    assert w[0, 0] == 1 and w[17, 160] == 1 and w[17, 159] == 23 / 24
    E = R.band_energies(np.ones((1, 161), complex))
    assert np.isclose(E.sum(), 161 + w[0].sum() + w[17].sum())


def test_floor_on_a_single_tone():
    t = np.arange(160 * 4)
    s = np.rint(20000 * np.sin(2 * np.pi * 1000 * t / 16000)).astype(np.int16)
    Ly = R.log_floor(R.band_energies(R.spectrum(R.windowed_frames(R.preemphasis(s), 4))))
    raw = np.log10(1e-2 + R.band_energies(R.spectrum(R.windowed_frames(R.preemphasis(s), 4))))
    assert (raw.max(axis=1, keepdims=True) - raw).max() > 8     # the tone alone would fall further than the floor lets it
    for f in range(1, 4):
        run_max = np.maximum.accumulate(Ly[f])
        assert (Ly[f] >= run_max - 8 - 1e-12).all()
        assert (np.diff(Ly[f]) >= -2.5 - 1e-12).all()
        assert (Ly[f] >= raw[f]).all()


@pytest.mark.parametrize("period", K.LOCKED_PERIODS)
def test_pitch_locks_on_pulse_trains(lpc_fn, period):
    for seed in K.PULSE_SEEDS:
        e = R.encode_trial(K.pulses(period, 160 * 12, seed), lpc_fn)
        f18 = e.features[3:, 18]
        got = np.floor(.1 + (50 * f18).astype(np.float64) + 100).astype(int)          # the decoder's formula (lpcnet_frame.hip)
        assert got.tolist() == [period] * 9, (period, seed, got)
        assert (e.features[3:, 19] > 0).all()


def test_white_noise_has_low_pitch_correlation(lpc_fn):
    for seed in (3, 4):
        e = R.encode_trial(K.white(160 * 12, seed), lpc_fn)
        assert (e.features[:, 19] < -0.2).all(), e.features[:, 19]


def test_lpc_whitens_a_resonance(lpc_fn):
    s = K.ar2(160 * 10, 50)
    e = R.encode_trial(s, lpc_fn)
    x = np.concatenate([np.zeros(96), R.preemphasis(s)])        # x[t] at index t + 96
    for i in range(1, 10):
        a = e.features[i, 20:].astype(np.float64)
        t = np.arange(160 * i - 80, 160 * i + 80)
        r = x[t + 96] + sum(a[j] * x[t + 96 - 1 - j] for j in range(16))
        assert (r ** 2).sum() < (x[t + 96] ** 2).sum(), i


def test_all_zero_audio(lpc_fn):
    e = R.encode_trial(K.zeros(160 * 6), lpc_fn)
    D = R.dct_table().astype(np.float64)
    c0 = 0.0
    for i in range(18):
        c0 = c0 + (-2.0) * D[i, 0]
    c0 = c0 * np.sqrt(2. / 18) - 4                              # Ly = log10(1e-2) = -2 in every band
    assert (e.cepstrum64[:, 0] == c0).all() and abs(c0 - (-6 * np.sqrt(2.) - 4)) < 1e-6
    assert np.abs(e.cepstrum64[:, 1:]).max() < 1e-14            # the other columns of D sum to zero
    assert np.array_equal(e.scores, np.zeros_like(e.scores))    # every score and weight is exactly 0
    assert (e.lags == 0).all()                                   # ties: the first index, so lag 256 twice, clamped to 510
    assert np.array_equal(e.features[:, 18], np.full(6, np.float32(0.01 * (510 - 200))))
    assert np.array_equal(e.features[:, 19], np.full(6, np.float32(-0.5)))
    assert e.margin >= 0.02 - 1e-12                              # the only strict comparisons left are between penalties


def test_a_trial_alone_equals_the_trial_in_a_list(lpc_fn, encoded):
    name, trials = K.cases()[2]
    encs, fo = encoded[name]
    assert fo.tolist() == np.concatenate([[0], np.cumsum([len(t) // 160 for t in trials])]).tolist()
    for k in (1, 2):
        alone = R.encode_trial(trials[k], lpc_fn)
        assert np.array_equal(alone.features, encs[k].features) and np.array_equal(alone.scores, encs[k].scores)


def test_short_trials_give_no_frames(lpc_fn):
    for n in (0, 1, 159):
        e = R.encode_trial(K.white(n, 60), lpc_fn)
        assert e.features.shape == (0, 36) and e.scores.shape == (0, 256)
    assert R.encode_trial(K.white(161, 61), lpc_fn).features.shape == (1, 36)


def test_case_table_margins(encoded):
    """The GPU test demands exact lags in every case: the reference's decisions must not hang on rounding."""
    for name, (encs, _) in encoded.items():
        for k, e in enumerate(encs):
            assert e.margin >= K.MIN_MARGIN, (name, k, e.margin)
            assert np.isfinite(e.features).all()
