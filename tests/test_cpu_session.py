"""Host side of the session path (trial lists, bad-channel patch, column statistics, normalization file) without a GPU:
the library loads on any machine and its host functions are held bit for bit to tests/golden/session.npz, which the
reference's own classes produced (tools/make_golden_session.py)."""
import os
import sys

import numpy as np
import pytest

from dss_amd import _lib, electrodes, hga, session

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))


def _patches(g):
    off = g["patch_off"]
    return [(int(d), g["patch_cols"][off[k]:off[k + 1]]) for k, d in enumerate(g["patch_dst"])]


def _corrected(g):
    out = g["frames"].copy()
    out[:, g["patch_dst"]] = g["corrected_columns"]
    return out


def _grids():
    speech = np.flip(np.arange(64, dtype=np.int16).reshape((8, 8)) + 1, axis=0)
    motor = np.flip(np.arange(64, dtype=np.int16).reshape((8, 8)) + 65, axis=0)
    return [speech, motor], np.arange(128) + 1


def test_fixture_covers_the_edge_cases(golden):
    g = golden("session.npz")
    assert "reference classes" in str(g["provenance"]) and "h5py placeholder untouched" in str(g["provenance"])
    lengths = [stop + 40 - start for start, stop in g["trials"]]
    assert any(40 < n < 50 for n in lengths) and 50 in lengths and any(n % 10 for n in lengths)
    assert g["frame_counts"].max() > 128 and g["frame_counts"].sum() == len(g["frames"])
    spans = sorted((s, e + 40) for s, e in g["trials"])
    assert any(a[1] > b[0] for a, b in zip(spans, spans[1:]))                 # two trials share recording rows
    sizes = np.diff(g["patch_off"])
    assert 8 in sizes and 3 in sizes and (g["patch_dst"] >= 64).any()


def test_neighbour_patches_equal_the_reference_class(golden):
    g = golden("session.npz")
    grids, layout = _grids()
    corrected = list(g["bad_channels"]) + list(g["contaminated_channels"])
    got = electrodes.neighbour_patches(corrected, grids, layout)
    want = _patches(g)
    assert [d for d, _ in got] == [d for d, _ in want]
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(got, want))
    assert all(np.array_equal(a[1], b[1]) and a[0] == b[0] for a, b in
               zip(session.offline_patches(g["bad_channels"], g["contaminated_channels"]), want))

    class Correction:                      # duck-typed BadChannelCorrection: .patches = [(np.where(...)[0], indices)]
        patches = [(np.array([d]), nb) for d, nb in want]
    assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(electrodes.patches_from_correction(Correction), want))


def test_frontend_128_reproduces_the_reference_car(golden):
    from ecog_chain_oracle import reference_chain
    ec = golden("ecog_chain.npz")
    both, car, speech = reference_chain()
    src, gof, comp = electrodes.frontend_from_transforms(both, car, None)
    assert src.shape == (128,) and gof.shape == (128,) and [len(c) for c in comp] == [60, 64]
    raw = ec["raw"]
    got = np.empty((len(raw), 128))
    for c in range(128):                    # what hga_frontend_kernel evaluates: sequential mean in list order
        acc = np.zeros(len(raw))
        for col in comp[gof[c]]:
            acc = acc + raw[:, col]
        got[:, c] = raw[:, src[c]] - acc / len(comp[gof[c]])
    assert np.array_equal(got, ec["after_car"])
    # the table-built form session.py configures is the same description; the three-transform form is unchanged
    a = session.offline_frontend()
    assert np.array_equal(a[0], src) and np.array_equal(a[1], gof) and all(np.array_equal(p, q) for p, q in zip(a[2], comp))
    b = electrodes.frontend_from_transforms(both, car, speech)
    assert np.array_equal(b[0], electrodes.reference_frontend()[0]) and len(b[0]) == 64


def test_host_patch_and_statistics_are_exact(golden):
    g = golden("session.npz")
    # the reference corrects trial by trial (a post-transform of extract_features), and numpy sums the 8 neighbours of a
    # ONE-frame call pairwise, of a longer one sequentially: the host function follows numpy by the frames it is given
    bounds = np.concatenate([[0], np.cumsum(g["frame_counts"])])
    got = np.concatenate([hga.apply_patches(g["frames"][a:b], _patches(g)) for a, b in zip(bounds, bounds[1:])])
    assert np.array_equal(got, _corrected(g))
    rng = np.random.default_rng(2)
    for n_rows in (1, 2, 3, 57):
        for k in (3, 5, 7, 8, 9, 12, 16, 17, 31):
            x = rng.standard_normal((n_rows, 128)) * 3.0 + 5.0
            cols = rng.permutation(128)
            want = x.copy()
            want[:, cols[0]] = np.mean(x[:, cols[1:k + 1]], axis=1)
            assert np.array_equal(hga.apply_patches(x, [(cols[0], cols[1:k + 1])]), want), (n_rows, k)
    assert np.array_equal(hga.column_stats(g["frames"]), np.vstack([g["mean_plain"], g["std_plain"]]))
    assert np.array_equal(hga.column_stats(got), np.vstack([g["mean"], g["std"]]))
    x = np.random.default_rng(1).standard_normal((5003, 128)) * 3.0 + 5.0     # the size numpy's order was established on
    assert np.array_equal(hga.column_stats(x), np.vstack([x.mean(axis=0), x.std(axis=0)]))
    one = x[:1]
    assert np.array_equal(hga.column_stats(one), np.vstack([one.mean(axis=0), one.std(axis=0)]))


def test_trial_frames_edge_lengths(golden):
    g = golden("session.npz")
    # frame 50 rows, shift 10: CASE 2 gives one frame for 11..49 rows, CASE 1 floor((n - 50) / 10) + 1 from 50 on
    for n, want in ((11, 1), (45, 1), (49, 1), (50, 1), (59, 1), (60, 2), (1279, 123), (1330, 129), (1340, 130), (1357, 131)):
        assert hga.trial_frames(n) == want, n
    for n in (10, 1, 0, -5):
        with pytest.raises(_lib.DssError):
            hga.trial_frames(n)
    ranges = session.trial_ranges(g["trials"], int(g["fs"][0]))
    assert [hga.trial_frames(n) for _, n in ranges] == g["frame_counts"].tolist()
    assert hga.check_trials(int(g["recording_seed"][1]), ranges) == len(g["frames"])
    assert hga.check_trials(100, []) == 0


def test_every_argument_check_returns_its_error():
    L = _lib.load()
    for trials in ([(0, 10)], [(-1, 100)], [(951, 50)], [(0, 100), (10**12, 50)], [(0, -3)]):
        with pytest.raises(_lib.DssError):
            hga.check_trials(1000, trials)
    assert hga.check_trials(1000, [(950, 50), (0, 1000)]) == 1 + 96
    start = np.zeros(1, np.int64)
    length = np.full(1, 60, np.int32)
    assert L.dss_hga_check_trials(1000, 0.05, 0.01, 100, -1, start.ctypes.data, length.ctypes.data) < 0
    assert L.dss_hga_check_trials(1000, 0.05, 0.01, 100, 1, None, None) < 0
    assert b"trial" in L.dss_last_error()
    x = np.zeros((3, 8))
    for bad in ([(8, [1, 2])], [(-1, [1])], [(0, [1, 8])], [(0, [])], [(0, [1]), (0, [2])], [(0, [1]), (1, [2])]):
        with pytest.raises(_lib.DssError):
            hga.apply_patches(x, bad)
    with pytest.raises(_lib.DssError):
        hga.column_stats(np.zeros((0, 4)))
    # the handle forms refuse a missing handle instead of faulting
    assert L.dss_hga_trial_frames(None, 100) < 0 and L.dss_hga_set_patches(None, 0, None, None, None) < 0
    assert L.dss_hga_extract_trials(None, None, 0, 0, None, None, None) < 0
    assert L.dss_hga_extract_trials_dev(None, None, 0, 0, None, None, None, 1, None) < 0


def test_save_normalization_round_trip(tmp_path, golden):
    g = golden("session.npz")
    stats = np.vstack([g["mean"], g["std"]])
    path = tmp_path / "normalization.npy"
    session.save_normalization(path, stats)
    want = tmp_path / "want.npy"
    np.save(want, np.vstack([g["mean"], g["std"]]))
    assert path.read_bytes() == want.read_bytes()
    statistics = np.load(path.as_posix())               # decode_online.py:90-92
    channel_means = statistics[0, :]
    channel_stds = statistics[1, :]
    assert np.array_equal(channel_means, g["mean"]) and np.array_equal(channel_stds, g["std"])
    with pytest.raises(ValueError):
        session.save_normalization(path, np.zeros((3, 128)))
