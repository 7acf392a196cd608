"""Host-side checks of the trial-list validation passes (dss_amd/validation.py, Part 8 of include/dss_hip.h): the trial borders,
the argument checks of the C ABI, the behaviour without a GPU, and the fixture condition of tests/test_gpu_validation.py."""
import ctypes as C

import numpy as np
import pytest

import lstm_reference as R
import validation_cases as V


def _count_trials(trial_ids):
    """SequentialSpeechTrials._count_trials (local/training.py:61-63)."""
    return len(np.where(trial_ids[:-1] != trial_ids[1:])[0]) + 1


def test_trial_bounds_docstring_example():
    """The example of training.py:69, seq [4, 4, 4, 3, 3, 3, -3, -3, -3, 5, 5, 5, -5, -5, -5, 5, 5, 5]: its borders [0, 3, 6, 9, 12,
    15, 18] make SIX trials (what _count_trials returns for it), and rows 9 .. 12, which that docstring names, are the fourth of
    them (index 3; the docstring's "n=4" counts from one although it says zero-indexed)."""
    from dss_amd.validation import trial_bounds
    seq = np.array([4, 4, 4, 3, 3, 3, -3, -3, -3, 5, 5, 5, -5, -5, -5, 5, 5, 5])
    b = trial_bounds(seq)
    assert len(b) == 6 == _count_trials(seq)
    assert b[4][0] == 12 and b[3] == (9, 3)
    first, length = b[3]
    assert (first, first + length) == (9, 12)
    assert trial_bounds([]) == [] and trial_bounds([7]) == [(0, 1)]


def test_trial_bounds_nine_trials():
    """A list of nine trials of unequal lengths, repeated stimuli negated as prepare_corpus.get_trial_ids writes them (5, -5, 5 are
    three trials): the fourth is rows 9 .. 12 again, every border is where _count_trials counts one."""
    from dss_amd.validation import trial_bounds
    seq = np.repeat([4, 3, -3, 5, -5, 5, 1, -1, 1], [3, 3, 3, 3, 3, 3, 2, 1, 4])
    b = trial_bounds(seq)
    assert len(b) == 9 == _count_trials(seq)
    assert b[3] == (9, 3) and b[8] == (21, 4)
    assert sum(n for _, n in b) == len(seq) and all(b[k][0] + b[k][1] == b[k + 1][0] for k in range(8))


def test_trial_bounds_on_the_session_corpus(golden):
    from dss_amd import session
    from dss_amd.validation import trial_bounds
    g = golden("session.npz")
    trials = [tuple(int(v) for v in t) for t in g["trials"]][1:]
    ids = session.trial_ids(trials, ["ba", "ba", "SILENCE", "du", "du"], ["SILENCE", "ba", "du"], int(g["fs"][0]))
    b = trial_bounds(ids)
    assert len(b) == _count_trials(ids) == 5
    assert [n for _, n in b] == [int(w) for w in g["frame_counts"][1:]]
    assert b[0][0] == 0 and all(b[k][0] + b[k][1] == b[k + 1][0] for k in range(4)) and b[4][0] + b[4][1] == len(ids)


def _check(L, N, ranges, null=None):
    first = np.array([a for a, _ in ranges], np.int64)
    length = np.array([n for _, n in ranges], np.int32)
    total = C.c_longlong(-1)
    args = [first.ctypes.data, length.ctypes.data, C.byref(total)]
    if null is not None:
        args[null] = None
    return L.dss_trials_check(N, len(ranges), *args), total.value


def test_trials_check():
    from dss_amd import _lib
    L = _lib.load()
    assert _check(L, 100, [(50, 50), (0, 100), (10, 1), (10, 1), (99, 1)]) == (0, 153)          # overlapping, unordered, to the last row
    assert _check(L, V.N_ROWS, V.RANGES) == (0, sum(n for _, n in V.RANGES))
    assert _check(L, 100, []) == (0, 0)
    for bad, word in (([(0, 0)], b"frames"), ([(0, -3)], b"frames"), ([(-1, 5)], b"negative"), ([(96, 5)], b"behind"),
                      ([(0, 10), (100, 1)], b"behind"), ([(0, 101)], b"behind")):
        rc, _ = _check(L, 100, bad)
        assert rc == -1 and word in L.dss_last_error(), (bad, L.dss_last_error())
    for null in (0, 1, 2):
        assert _check(L, 100, [(0, 10)], null=null)[0] == -1 and b"null" in L.dss_last_error()
    first = np.zeros(1, np.int64)
    length = np.ones(1, np.int32)
    total = C.c_longlong(0)
    assert L.dss_trials_check(100, -1, first.ctypes.data, length.ctypes.data, C.byref(total)) == -1


def test_no_gpu_raises():
    from dss_amd import _lib
    from dss_amd.validation import decoder_validation, vad_validation
    L = _lib.load()
    if L.dss_device_count() > 0:
        pytest.skip("a GPU is present")
    x = V.corpus(1)[:40]
    ids = np.repeat([1, 2], 20)
    with pytest.raises(_lib.DssError):
        vad_validation(R.vad_state_dict(V.VAD_H, V.C, 1), x, np.zeros(40, bool), ids)
    with pytest.raises(_lib.DssError):
        decoder_validation(R.decoder_state_dict(V.DEC_H, V.C, 1), x, np.zeros((40, 20), np.float32), ids)
    # the reductions take no handle: they fail on their own
    one = np.ones(1, np.int32)
    assert L.dss_vad_score_trials_dev(1, 1, 1, 1, one.ctypes.data, 1, 1, None, None) == -2
    assert L.dss_dec_mse_trials_dev(1, 1, 20, 1, one.ctypes.data, 1, None) == -2


def test_foreign_architecture_is_refused_before_anything_runs():
    """No silent fallback: a state_dict that is not the reference's detector / decoder raises (with or without a GPU)."""
    from dss_amd import _lib
    from dss_amd.validation import decoder_validation, vad_validation
    sd = dict(R.vad_state_dict(V.VAD_H, V.C, 1))
    sd["extra.weight"] = sd["classifier.bias"]
    with pytest.raises((ValueError, _lib.DssError)):
        vad_validation(sd, V.corpus(1)[:8], np.zeros(8, bool), np.ones(8))
    with pytest.raises((ValueError, _lib.DssError)):
        decoder_validation(R.vad_state_dict(V.VAD_H, V.C, 1), V.corpus(1)[:8], np.zeros((8, 20), np.float32), np.ones(8))


@pytest.mark.parametrize("scale", [1, 4])
def test_fixture_has_no_near_tie(scale):
    """The condition under which tests/test_gpu_validation.py may demand equal labels on EVERY frame: on the float64 reference alone,
    no frame of any trial has |z1 - z0| <= 2 x bound(scale) -- zero frames left out."""
    z = V.vad_reference_logits(scale)
    assert z.shape == (sum(n for _, n in V.RANGES), 2)
    margin = np.abs(z[:, 1] - z[:, 0])
    print(f"x{scale}: smallest margin {margin.min():.3e}, 2 x bound {2 * R.bound(scale):.1e}, speech frames {(z[:, 1] > z[:, 0]).mean():.3f}")
    assert int((margin <= 2 * R.bound(scale)).sum()) == 0
    assert sorted({n for _, n in V.RANGES}) == [1, 3, 4, 5, 50, 251, 1500]
