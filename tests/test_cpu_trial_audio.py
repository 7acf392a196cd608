"""The loudness step of the reference's trial audio without a GPU: the restatement (tests/trial_audio_reference.py) against
Python's own ``audioop`` -- the C code pydub calls --, the library's two host functions (the functions its kernels apply)
against the restatement, the gain table against its formula, and tests/golden/trial_audio.npz
(tools/make_golden_trial_audio.py) against the restatement.

What is NOT pinned: that pydub's wrapper computes the two factors as ``dss_amd.trial_audio`` restates them.  pydub is not
installed where this was written; ``test_pydub_itself`` runs the day it is (tests/golden/TRIAL_AUDIO.md)."""
import ctypes as C
import hashlib
import math
import os
import re

import numpy as np
import pytest

import trial_audio_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dss_avad_peak_host", "dss_avad_scale_host", "dss_avad_peak_tile", "dss_avad_set_gain", "dss_avad_prepare_trials",
       "dss_avad_prepare_trials_dev")
ALL_INT16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)


def _factors():
    from dss_amd import trial_audio
    table = trial_audio.pydub_gain_table()
    return [trial_audio.post_gain()] + [float(table[p]) for p in (1, 2, 3, 17, 9000, 32767, 32768)] + [0.5, 1.5, 2.3]


def _audio(g):
    from dss_amd.synthetic import synthetic_speech_audio
    seed, n, fs, z0, z1 = (int(v) for v in g["audio_seed"])
    loud = synthetic_speech_audio(seed, n, fs)
    loud[z0:z1] = 0
    wav = np.concatenate([loud, np.trunc(loud.astype(np.float64) * float(g["quiet_scale"])).astype(np.int16)])
    assert hashlib.sha256(wav.tobytes()).digest() == g["audio_sha"].tobytes()
    return wav


def test_entry_points_are_declared_and_exported():
    from dss_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dss_hip.h")).read(), flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert L.dss_avad_peak_tile() >= 256


def test_restatement_equals_audioop_on_every_int16_value():
    audioop = pytest.importorskip("audioop")                 # leaves the standard library in 3.13
    data = ALL_INT16.tobytes()
    assert audioop.max(data, 2) == ref.peak(ALL_INT16) == 32768
    saturated = 0
    for f in _factors():
        want = np.frombuffer(audioop.mul(data, 2, f), dtype=np.int16)
        got = ref.scale(ALL_INT16, f)
        assert np.array_equal(got, want), f
        saturated += int(np.sum(want == 32767) > 1) + int(np.sum(want == -32768) > 1)
    assert saturated >= 6                                    # 1.5, 2.3 and the small peaks' factors reach both clamps
    for x in (np.array([-32768], np.int16), np.array([0, 0], np.int16), np.array([5, -7, 3], np.int16), np.zeros(0, np.int16)):
        assert ref.peak(x) == (audioop.max(x.tobytes(), 2) if len(x) else 0)


def test_two_gains_are_not_one(golden):
    """A folded gain (one product) must not pass for pydub's two: on the fixture's trials it changes 9 % of the nonzero
    samples or more (the loud trials, whose samples are mostly small room noise, change least)."""
    g = golden("trial_audio.npz")
    wav = _audio(g)
    table, post = ref.gain_table(), ref.post_gain()
    seen = 0
    for (first, n, lead, silence), pk in zip(g["trials"], g["peaks"]):
        if silence or pk == 0:
            continue
        c = ref.cut(wav, int(first), int(n))
        loud = c[c != 0]                                     # zero stays zero under any gain
        if len(loud) < 100:
            continue
        two = ref.scale(ref.scale(loud, table[pk]), post)
        one = ref.scale(loud, table[pk] * post)
        differ = float(np.mean(two != one))
        print("trial at", int(first), "peak", int(pk), ": one folded product changes %.1f %% of the nonzero samples" % (100 * differ))
        assert differ > 0.05, int(first)                     # far more than a hash or a sample-for-sample comparison can miss
        seen += 1
    assert seen >= 8


def test_library_host_functions_equal_the_restatement():
    from dss_amd import _lib, trial_audio
    for f in _factors() + [0.0, 1.0, 1e-9, 32768.0, 1e300, -1.0, -2.3]:
        assert np.array_equal(trial_audio.scale_host(ALL_INT16, f), ref.scale(ALL_INT16, f)), f
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 7, 4095, 4096, 4097, 70001):
        x = rng.integers(-3000, 3000, n).astype(np.int16)
        assert trial_audio.peak_host(x) == ref.peak(x)
    for x in ([-32768], [32767, -32767], [0, 0, 0], [-1], [1, -32768, 32767]):
        assert trial_audio.peak_host(np.array(x, np.int16)) == ref.peak(np.array(x, np.int16))
    L = _lib.load()
    with pytest.raises(_lib.DssError, match="not finite"):
        trial_audio.scale_host(ALL_INT16, float("nan"))
    with pytest.raises(_lib.DssError, match="not finite"):
        trial_audio.scale_host(ALL_INT16, float("inf"))
    with pytest.raises(ValueError):
        trial_audio.peak_host(np.zeros(4, np.int32))
    assert L.dss_avad_peak_host(None, 5) == -1 and L.dss_avad_scale_host(None, 5, 1.0, None) == -1
    assert L.dss_avad_peak_host(None, 0) == 0


def test_table_equals_the_formula():
    from dss_amd import trial_audio
    table = trial_audio.pydub_gain_table()
    assert table.dtype == np.float64 and table.shape == (32769,) and table[0] == 1.0
    assert np.array_equal(table, ref.gain_table())
    target = 32768 * 10 ** (-0.1 / 20)
    for p in (1, 2, 3, 17, 9000, 32767, 32768):
        assert table[p] == 10 ** (float(20 * math.log(target / p, 10)) / 20)
        assert abs(table[p] * p - target) <= 1e-9 * target                  # the factor brings the peak to the headroom
    assert np.all(np.diff(table[1:]) < 0) and np.all(np.isfinite(table)) and table[32768] < 1.0 < table[32000]
    assert trial_audio.post_gain() == 10 ** (-3.0 / 20) == ref.post_gain()
    assert trial_audio.post_gain(-6.0) == 10 ** (-6.0 / 20)
    other = trial_audio.pydub_gain_table(1.0)
    assert other[0] == 1.0 and np.all(other[1:] < table[1:])


def test_set_gain_refuses_bad_tables():
    from dss_amd import _lib, trial_audio
    L = _lib.load()
    table = trial_audio.pydub_gain_table()
    # the data is judged before the handle, so no device is needed: a good table without a handle fails on the handle
    assert L.dss_avad_set_gain(None, table.ctypes.data, 0.7) == -1 and b"no handle" in L.dss_last_error()
    assert L.dss_avad_set_gain(None, None, 0.7) == -1
    for k, bad in ((5, float("nan")), (0, -1.0), (32768, float("inf")), (17, -1e-300)):
        t = table.copy()
        t[k] = bad
        assert L.dss_avad_set_gain(None, t.ctypes.data, 0.7) == -1
        assert b"peak %d is negative or not finite" % k in L.dss_last_error(), k
    for post in (float("nan"), -0.5, float("inf")):
        assert L.dss_avad_set_gain(None, table.ctypes.data, post) == -1 and b"post gain" in L.dss_last_error()


def test_fixture_reproduces_from_the_restatement(golden):
    g = golden("trial_audio.npz")
    prov = str(g["provenance"])
    assert "audioop" in prov and "reference classes" in prov and "h5py placeholder untouched" in prov and "pydub itself not installed" in prov
    wav = _audio(g)
    table, post = ref.gain_table(float(g["headroom_db"])), ref.post_gain()
    assert float(g["post_gain"]) == post
    t = g["trials"]
    assert len(t) == 13 and t[:, 3].sum() == 2 and np.all(t[:, 2] == 256)
    for k, (first, n, lead, silence) in enumerate(t):
        x, pk = ref.prepared_trial(wav, int(first), int(n), int(lead), not silence, table, post)
        assert pk == g["peaks"][k], k
        assert g["factors"][k] == (1.0 if silence else table[pk]), k
        assert ref.sha(x) == g["prepared_sha"][k].tobytes(), k
        assert not x[:lead].any()
    # the cases the fixture is there for
    assert 0 in g["peaks"].tolist() and any(f % 2 for f in t[:, 0])                       # digital silence; an odd first sample
    assert any(n < asked for (_, asked), n in zip(g["trials_asked"], t[:, 1]))            # one trial clamped at the end of the audio
    assert int(t[-1, 0] + t[-1, 1]) == len(wav)
    assert g["frame_counts"].tolist() == [(int(n) - 800) // 160 + 1 for n in t[:, 1]]
    bounds = np.concatenate([[0], np.cumsum(g["frame_counts"])])
    moved = [int(np.sum(g["labels"][a:b] != g["labels_plain"][a:b])) for a, b in zip(bounds, bounds[1:])]
    assert sum(moved) >= 1 and all(m == 0 for m, f in zip(moved, t[:, 0]) if f < int(g["audio_seed"][1]))   # only quiet trials move
    for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
        assert np.min(np.abs(g["log_energy"][a:b] - g["thresholds"][k])) >= 0.8, k
        if t[k, 3]:
            assert not g["labels"][a:b].any()


def test_restatement_energies_agree_with_the_reference(golden):
    """The restatement's own deviation from the fixture's log energies: one of the two figures behind the GPU test's bound."""
    import acoustic_vad_reference as vref
    from dss_amd import acoustic_vad
    g = golden("trial_audio.npz")
    wav = _audio(g)
    table, post = ref.gain_table(), ref.post_gain()
    window, mel = acoustic_vad.hann(800), acoustic_vad.mel_filterbank(401, 40, 16000)
    bounds = np.concatenate([[0], np.cumsum(g["frame_counts"])])
    worst = worst_thr = 0.0
    for k, (first, n, lead, silence) in enumerate(g["trials"]):
        x, _ = ref.prepared_trial(wav, int(first), int(n), int(lead), not silence, table, post)
        le = vref.log_energy(x, window, mel)
        a, b = bounds[k], bounds[k + 1]
        worst = max(worst, float(np.max(np.abs(le - g["log_energy"][a:b]))))
        labels, thr, _ = vref.vote(le)
        worst_thr = max(worst_thr, abs(thr - float(g["thresholds"][k])))
        if silence:
            labels[:] = False
        assert np.array_equal(labels, g["labels"][a:b]), k
    print("restatement vs reference on the prepared audio, max |log energy difference|:", worst, "threshold:", worst_thr)
    assert worst <= 2e-12 and worst_thr <= 2e-12


def test_session_signatures_keep_their_defaults():
    import inspect
    from dss_amd import session
    from dss_amd.acoustic_vad import AcousticVadGPU
    assert inspect.signature(session.session_corpus).parameters["normalize_audio"].default is False
    assert inspect.signature(session.session_vad_labels).parameters["normalize"].default is False
    assert list(inspect.signature(session.session_trial_audio).parameters)[:7] == ["wav", "trials", "stimulus_labels", "fs", "fs_audio",
                                                                                   "shift_seconds", "norm_db"]
    for name in ("labels_trials", "labels_trials_torch", "prepared_audio_trials", "prepared_audio_trials_torch"):
        assert inspect.signature(getattr(AcousticVadGPU, name)).parameters["normalize"].default is None


def test_pydub_itself():
    """The unpinned part, stated: runs where pydub is installed, skipped elsewhere."""
    pydub = pytest.importorskip("pydub")
    from pydub import effects
    from dss_amd import trial_audio
    from dss_amd.synthetic import synthetic_speech_audio
    table, post = trial_audio.pydub_gain_table(), trial_audio.post_gain()
    wav = synthetic_speech_audio(7109, 120000)
    for x in (wav[60000:100640], np.trunc(wav[60000:100640] * 0.02).astype(np.int16), np.array([-32768, 5, 7], np.int16),
              np.array([1, 0, -1], np.int16), np.zeros(100, np.int16)):
        seg = pydub.AudioSegment(x.tobytes(), frame_rate=16000, sample_width=2, channels=1)
        want = np.array(effects.normalize(seg).apply_gain(-3.0).get_array_of_samples(), dtype=np.int16)
        assert np.array_equal(ref.scale(ref.scale(x, table[ref.peak(x)]), post), want)
