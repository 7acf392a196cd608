"""A session's trial list in one call on the GPU (dss_hga_extract_trials*), held to tests/golden/session.npz, which the
reference's own classes produced (tools/make_golden_session.py), and to the streaming extractor as a second witness.

Host-buffer path: array_equal.  Device path: frames within 1 ulp (OCML log, the bound of dss_hga_extract_dev); patch and
statistics array_equal to numpy on the device's own frames.  Device statistics against the fixture, measured on an MI355X
over the 277 fixture frames (device frames differ from the fixture's by at most 1 ulp of the log): the mean came out equal
(relative difference 0), the std differs by at most 1.355e-16 relative, with and without patches.  The bound is 4x the
larger measured figure, 5.42e-16, and must stay under the cap N * 2^-53 = 3.08e-14, the worst case of a sequential sum.
"""
import hashlib
import math

import numpy as np
import pytest

from dss_amd.synthetic import synthetic_ecog

pytestmark = pytest.mark.gpu

STATS_REL_BOUND = 4 * 1.355e-16     # 4 x the measured figure (docstring); the cap is checked in the test


@pytest.fixture(scope="module")
def fx(golden):
    from dss_amd import session
    g = golden("session.npz")
    seed, T, c_raw = (int(v) for v in g["recording_seed"])
    rec = synthetic_ecog(seed, T, c_raw)
    assert hashlib.sha256(rec.tobytes()).digest() == g["recording_sha"].tobytes()
    off = g["patch_off"]
    patches = [(int(d), g["patch_cols"][off[k]:off[k + 1]]) for k, d in enumerate(g["patch_dst"])]
    corrected = g["frames"].copy()
    corrected[:, g["patch_dst"]] = g["corrected_columns"]
    fs = int(g["fs"][0])
    return {"g": g, "rec": rec, "c_raw": c_raw, "fs": fs, "patches": patches, "corrected": corrected,
            "trials": [tuple(int(v) for v in t) for t in g["trials"]], "ranges": session.trial_ranges(g["trials"], fs),
            "bounds": np.concatenate([[0], np.cumsum(g["frame_counts"])])}


def _extractor(fx, patches=False):
    from dss_amd import session
    ex = session.session_extractor(fx["c_raw"], fx["fs"])
    if patches:
        ex.set_patches(fx["patches"])
    return ex


def test_host_path_equals_the_reference_chain(fx):
    ex = _extractor(fx)
    got = ex.extract_trials(fx["rec"], fx["ranges"])
    assert got.shape == fx["g"]["frames"].shape and np.array_equal(got, fx["g"]["frames"])
    ex.set_patches(fx["patches"])
    assert np.array_equal(ex.extract_trials(fx["rec"], fx["ranges"]), fx["corrected"])
    ex.set_patches(None)
    assert np.array_equal(ex.extract_trials(fx["rec"], fx["ranges"]), fx["g"]["frames"])
    # the z-score follows the patch (ZScoreNormalization behind BadChannelCorrection), same two IEEE operations
    ex.set_patches(fx["patches"])
    ex.set_zscore(fx["g"]["mean"], fx["g"]["std"])
    assert np.array_equal(ex.extract_trials(fx["rec"], fx["ranges"]), (fx["corrected"] - fx["g"]["mean"]) / fx["g"]["std"])


def test_session_functions_equal_the_fixture(fx):
    from dss_amd import session
    g = fx["g"]
    assert np.array_equal(session.session_features(fx["rec"], fx["trials"], fx["fs"]), g["frames"])
    stats = session.normalization_statistics(fx["rec"], fx["trials"], fx["fs"])
    assert stats.shape == (2, 128) and np.array_equal(stats, np.vstack([g["mean_plain"], g["std_plain"]]))
    stats = session.normalization_statistics(fx["rec"], fx["trials"], fx["fs"], bad_channels=list(g["bad_channels"]),
                                             contaminated_channels=list(g["contaminated_channels"]))
    assert np.array_equal(stats, np.vstack([g["mean"], g["std"]]))


def test_one_call_equals_the_streaming_extractor_trial_by_trial(fx):
    from dss_amd import session
    from dss_amd.hga import HgaExtractorGPU
    one_call = _extractor(fx).extract_trials(fx["rec"], fx["ranges"])
    old = HgaExtractorGPU(1, 128, fs=fx["fs"])
    old.set_frontend(fx["c_raw"], *session.offline_frontend())
    for (start, n), a, b in zip(fx["ranges"], fx["bounds"], fx["bounds"][1:]):
        old.reset()
        assert np.array_equal(old.extract_raw(fx["rec"][start:start + n].copy())[0], one_call[a:b]), (start, n)
    # the handle's streaming state is neither read nor written by a trial call
    x = synthetic_ecog(77, 400, fx["c_raw"])
    chunks = [(0, 40), (40, 97), (97, 200), (200, 240), (240, 400)]
    disturbed, calm = _extractor(fx), _extractor(fx)
    for k, (a, b) in enumerate(chunks):
        if k in (1, 3):
            assert np.array_equal(disturbed.extract_trials(fx["rec"], fx["ranges"]), one_call)
        assert np.array_equal(disturbed.extract_raw(x[a:b])[0], calm.extract_raw(x[a:b])[0]), k


def test_device_path(fx):
    import torch
    from dss_amd import hga
    g = fx["g"]
    rec = torch.from_numpy(fx["rec"]).cuda()
    ex = _extractor(fx)
    dev = ex.extract_trials_torch(rec, fx["ranges"])
    torch.cuda.synchronize()
    frames = dev.cpu().numpy()
    ulp = np.abs(frames - g["frames"]) / np.spacing(np.abs(g["frames"]))
    print("device frames vs fixture: max ulp", ulp.max())
    assert ulp.max() <= 1.0
    power = ex.extract_trials_torch(rec, fx["ranges"], apply_log=False).cpu().numpy()
    # everything but the log is exact (math.log is the host libm's, which the reference's Cython module calls; np.log is not)
    assert np.array_equal(np.vectorize(math.log)(power), g["frames"])
    # patch on the device: numpy's class on the device's own frames, trial by trial as the reference applies it
    ex.set_patches(fx["patches"])
    patched_dev = ex.extract_trials_torch(rec, fx["ranges"])
    patched = patched_dev.cpu().numpy()
    want = np.concatenate([hga.apply_patches(frames[a:b], fx["patches"]) for a, b in zip(fx["bounds"], fx["bounds"][1:])])
    assert np.array_equal(patched, want)
    want_np = frames.copy()
    for a, b in zip(fx["bounds"], fx["bounds"][1:]):
        for dst, nb in fx["patches"]:
            want_np[a:b, dst] = np.mean(frames[a:b][:, nb], axis=1)
    assert np.array_equal(patched, want_np)
    ulp = np.abs(patched - fx["corrected"]) / np.spacing(np.abs(fx["corrected"]))
    print("device corrected frames vs fixture: max ulp", ulp.max())
    # statistics on the device: numpy's order, exact on the device's own frames
    N = len(frames)
    cap = N * 2.0 ** -53
    assert STATS_REL_BOUND < cap
    for name, t, host, want_mean, want_std in (("plain", dev, frames, g["mean_plain"], g["std_plain"]),
                                               ("corrected", patched_dev, patched, g["mean"], g["std"])):
        stats = hga.column_stats_torch(t).cpu().numpy()
        assert np.array_equal(stats, np.vstack([host.mean(axis=0), host.std(axis=0)])), name
        rel_mean = np.max(np.abs(stats[0] - want_mean) / np.abs(want_mean))
        rel_std = np.max(np.abs(stats[1] - want_std) / np.abs(want_std))
        print(f"device statistics vs fixture ({name}): rel mean {rel_mean:.3e} rel std {rel_std:.3e} cap {cap:.3e}")
        assert rel_mean <= STATS_REL_BOUND and rel_std <= STATS_REL_BOUND, name
    # z-score behind the patch on the device: the same two IEEE operations on the device's frames
    ex.set_zscore(g["mean"], g["std"])
    assert np.array_equal(ex.extract_trials_torch(rec, fx["ranges"]).cpu().numpy(), (patched - g["mean"]) / g["std"])
    ex.set_patches(None)                     # without patches the z-score is the trial kernel's own epilogue
    assert np.array_equal(ex.extract_trials_torch(rec, fx["ranges"]).cpu().numpy(), (frames - g["mean"]) / g["std"])


def test_order_and_list_sizes(fx):
    ex = _extractor(fx)
    base = ex.extract_trials(fx["rec"], fx["ranges"])
    per_trial = [base[a:b] for a, b in zip(fx["bounds"], fx["bounds"][1:])]
    order = np.random.default_rng(5).permutation(len(fx["ranges"]))
    got = ex.extract_trials(fx["rec"], [fx["ranges"][i] for i in order])
    pos = 0
    for i in order:
        assert np.array_equal(got[pos:pos + len(per_trial[i])], per_trial[i]), i
        pos += len(per_trial[i])
    assert pos == len(got)
    for i, r in enumerate(fx["ranges"]):                                     # n_trials = 1
        assert np.array_equal(ex.extract_trials(fx["rec"], [r]), per_trial[i])
    assert ex.extract_trials(fx["rec"], []).shape == (0, 128)
    # n_trials = 300: seeded windows of 45 .. 700 rows anywhere in the recording, many overlapping; repeated ranges agree
    rng = np.random.default_rng(6)
    T = len(fx["rec"])
    many = []
    for _ in range(300):
        n = int(rng.integers(45, 700))
        many.append((int(rng.integers(0, T - n)), n))
    many[17], many[250] = fx["ranges"][2], fx["ranges"][0]
    got = ex.extract_trials(fx["rec"], many)
    counts = [ex.trial_frames(n) for _, n in many]
    assert len(got) == sum(counts)
    b = np.concatenate([[0], np.cumsum(counts)])
    assert np.array_equal(got[b[17]:b[18]], per_trial[2]) and np.array_equal(got[b[250]:b[251]], per_trial[0])
    for i in (0, 99, 299):
        assert np.array_equal(ex.extract_trials(fx["rec"], [many[i]]), got[b[i]:b[i + 1]])
    # a plain (no front end) extractor takes the trial list too: 5 channels, an odd count, against the streaming path
    from dss_amd.hga import HgaExtractorGPU
    x = synthetic_ecog(78, 900, 5)
    plain, old = HgaExtractorGPU(1, 5), HgaExtractorGPU(1, 5)
    lst = [(0, 900), (13, 45), (400, 333)]
    got = plain.extract_trials(x, lst)
    pos = 0
    for s, n in lst:
        old.reset()
        want = old.extract(x[s:s + n].copy())[0]
        assert np.array_equal(got[pos:pos + len(want)], want)
        pos += len(want)


def test_argument_checks_leave_nothing_to_the_device(fx):
    from dss_amd import _lib
    ex = _extractor(fx)
    T = len(fx["rec"])
    for bad in ([(0, 10)], [(T - 49, 50)], [(-1, 60)], [(0, 60), (T, 60)]):
        with pytest.raises(_lib.DssError):
            ex.extract_trials(fx["rec"], bad)
    for bad in ([(128, [0])], [(0, [1]), (1, [2])], [(0, [])]):
        with pytest.raises(_lib.DssError):
            ex.set_patches(bad)
    with pytest.raises(ValueError):
        ex.extract_trials(fx["rec"][:, :128], fx["ranges"])
    assert ex.trial_frames(45) == 1 and ex.trial_frames(1357) == 131
    with pytest.raises(_lib.DssError):
        ex.trial_frames(10)
    assert np.array_equal(ex.extract_trials(fx["rec"], fx["ranges"]), fx["g"]["frames"])      # still serviceable
