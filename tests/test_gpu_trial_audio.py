"""The trial audio as the reference prepares it, on the GPU (dss_avad_set_gain, dss_avad_prepare_trials*): peak, pydub's two
gains, the shift; the labels of that audio; the audio itself.  Held to tests/golden/trial_audio.npz, which Python's own audioop
and the reference's own EnergyBasedVad produced (tools/make_golden_trial_audio.py), and beyond it to the numpy restatement in
tests/trial_audio_reference.py.  Integers (audio, peaks, labels) are compared with array_equal throughout.

The normalised call is tied to the kernel that tests/test_gpu_acoustic_vad.py already pins at tolerance 0: its energies,
thresholds and labels equal, bit for bit, those of the plain call on the prepared audio.

Log energy and threshold against the reference (values between -1290 and 97), by the rule of tests/test_gpu_acoustic_vad.py:
measured on an MI355X over the 2367 fixture frames, the kernel's worst deviation from the fixture is 9.09e-13 (threshold:
9.09e-13); the numpy restatement's, measured on the CPU (tests/test_cpu_trial_audio.py prints it), is 1.05e-12 (threshold
1.14e-13).  The bound is 4x the larger of the two, 4.24e-12, and must stay under the cap 1e-10.
"""
import hashlib

import numpy as np
import pytest

import acoustic_vad_reference as vref
import trial_audio_reference as ref
from dss_amd.synthetic import synthetic_ecog, synthetic_speech_audio

pytestmark = pytest.mark.gpu

MEASURED_KERNEL = 9.10e-13          # max |log energy - fixture| of the normalised call on an MI355X
MEASURED_RESTATEMENT = 1.06e-12     # the same figure of the numpy restatement on the prepared audio (CPU)
LOG_ENERGY_BOUND = 4 * max(MEASURED_KERNEL, MEASURED_RESTATEMENT)
LEAD = 256


@pytest.fixture(scope="module")
def tables():
    return ref.gain_table(), ref.post_gain()


@pytest.fixture(scope="module")
def fx(golden, tables):
    g = golden("trial_audio.npz")
    seed, n, fs, z0, z1 = (int(v) for v in g["audio_seed"])
    loud = synthetic_speech_audio(seed, n, fs)
    loud[z0:z1] = 0
    wav = np.concatenate([loud, np.trunc(loud.astype(np.float64) * float(g["quiet_scale"])).astype(np.int16)])
    assert hashlib.sha256(wav.tobytes()).digest() == g["audio_sha"].tobytes()
    t = g["trials"]
    ranges = [(int(a), int(b)) for a, b in t[:, :2]]
    lead = [int(v) for v in t[:, 2]]
    silence = [bool(v) for v in t[:, 3]]
    prepared, peaks, offsets = ref.prepared_list(wav, ranges, lead, [not s for s in silence], *tables)
    return {"g": g, "wav": wav, "ranges": ranges, "lead": lead, "silence": silence, "prepared": prepared, "peaks": peaks,
            "offsets": offsets, "bounds": np.concatenate([[0], np.cumsum(g["frame_counts"])])}


@pytest.fixture(scope="module")
def vad(tables):
    from dss_amd import trial_audio
    from dss_amd.acoustic_vad import AcousticVadGPU
    assert np.array_equal(trial_audio.pydub_gain_table(), tables[0]) and trial_audio.post_gain() == tables[1]
    v = AcousticVadGPU()
    v.set_gain()
    yield v
    v.close()


def _plain_on_prepared(v, prepared, offsets, lengths, lead, silence=None):
    """Today's un-normalised call on prepared audio laid out trial after trial, with the same lengths and leads."""
    lead = np.broadcast_to(np.asarray(lead), (len(lengths),))
    ranges = [(int(off) + int(ld), int(n)) for off, n, ld in zip(offsets, lengths, lead)]
    return v.labels_trials(prepared, ranges, lead=[int(x) for x in lead], silence=silence, return_energy=True)


# ---- 1: the fixture's audio and peaks -------------------------------------------------------------------------------------
def test_fixture_audio_and_peaks_in_one_call(fx, vad):
    g = fx["g"]
    audio, peaks = vad.prepared_audio_trials(fx["wav"], fx["ranges"], lead=fx["lead"], normalize=True, silence=fx["silence"],
                                             return_peaks=True)
    assert audio.dtype == np.int16 and peaks.dtype == np.int32
    assert np.array_equal(peaks, g["peaks"]) and np.array_equal(peaks, fx["peaks"])
    off = fx["offsets"]
    for k in range(len(fx["ranges"])):
        assert hashlib.sha256(audio[off[k]:off[k + 1]].tobytes()).digest() == g["prepared_sha"][k].tobytes(), k
    assert np.array_equal(audio, fx["prepared"])                                    # sample for sample
    # without the flag the operator only shifts
    raw = vad.prepared_audio_trials(fx["wav"], fx["ranges"], lead=fx["lead"])
    want, _, _ = ref.prepared_list(fx["wav"], fx["ranges"], fx["lead"], [False] * len(fx["ranges"]), None, None)
    assert np.array_equal(raw, want) and not np.array_equal(raw, audio)


# ---- 2: tied to the pinned kernel at tolerance 0 ----------------------------------------------------------------------------
def test_normalised_call_equals_the_plain_call_on_the_prepared_audio(fx, vad):
    got = vad.labels_trials(fx["wav"], fx["ranges"], lead=fx["lead"], silence=fx["silence"], return_energy=True, normalize=True)
    audio = vad.prepared_audio_trials(fx["wav"], fx["ranges"], lead=fx["lead"], normalize=True, silence=fx["silence"])
    want = _plain_on_prepared(vad, audio, fx["offsets"], [n for _, n in fx["ranges"]], fx["lead"], fx["silence"])
    for a, b, what in zip(got, want, ("labels", "log energy", "threshold")):
        assert np.array_equal(a, b), what
    plain = vad.labels_trials(fx["wav"], fx["ranges"], lead=fx["lead"], silence=fx["silence"], return_energy=True)
    assert not np.array_equal(plain[1], got[1])                                     # the gain does change the energies
    assert np.array_equal(vad.labels_trials(fx["wav"], fx["ranges"], lead=fx["lead"], silence=fx["silence"], normalize=True), got[0])


# ---- 3: against the reference's fixture -------------------------------------------------------------------------------------
def test_fixture_labels_energies_and_thresholds(fx, vad):
    g = fx["g"]
    labels, le, thr = vad.labels_trials(fx["wav"], fx["ranges"], lead=fx["lead"], silence=fx["silence"], return_energy=True,
                                        normalize=True)
    assert labels.dtype == bool and np.array_equal(labels, g["labels"])             # every frame, none left out
    assert not np.array_equal(g["labels"], g["labels_plain"])                       # ... and the loudness step moved one
    plain = vad.labels_trials(fx["wav"], fx["ranges"], lead=fx["lead"], silence=fx["silence"])
    assert np.array_equal(plain, g["labels_plain"])
    worst = float(np.max(np.abs(le - g["log_energy"])))
    worst_thr = float(np.max(np.abs(thr - g["thresholds"])))
    print("normalised kernel vs reference, max |log energy difference|:", worst, "threshold:", worst_thr, "bound", LOG_ENERGY_BOUND)
    assert LOG_ENERGY_BOUND <= 1e-10
    assert worst <= LOG_ENERGY_BOUND
    assert worst_thr <= LOG_ENERGY_BOUND


# ---- 4: the smallest shapes that can go wrong -------------------------------------------------------------------------------
def _noise(n, seed, amp=40):
    return np.random.default_rng(seed).integers(-amp, amp + 1, n).astype(np.int16)


def _check(v, wav, ranges, lead, normalize, tables, silence=None, frames=True):
    """Audio and peaks against the restatement, from host buffers (where the first trial's first sample lands on an aligned
    address of the staging buffer) and device-resident (where `first` itself decides the alignment); labels, energies and
    thresholds against the plain call on that audio."""
    import torch
    n_trials = len(ranges)
    flags = [bool(x) for x in np.broadcast_to(np.asarray(normalize), (n_trials,))]
    if silence is not None:
        flags = [f and not s for f, s in zip(flags, silence)]
    want, want_peaks, offsets = ref.prepared_list(wav, ranges, lead, flags, *tables)
    audio, peaks = v.prepared_audio_trials(wav, ranges, lead=lead, normalize=flags, return_peaks=True)
    assert np.array_equal(peaks, want_peaks), (peaks, want_peaks)
    assert np.array_equal(audio, want)
    d_wav = torch.from_numpy(wav).cuda()
    d_audio, d_peaks = v.prepared_audio_trials_torch(d_wav, ranges, lead=lead, normalize=flags, return_peaks=True)
    assert np.array_equal(d_peaks.cpu().numpy(), want_peaks) and np.array_equal(d_audio.cpu().numpy(), want)
    if frames:
        got = v.labels_trials(wav, ranges, lead=lead, silence=silence, return_energy=True, normalize=flags)
        plain = _plain_on_prepared(v, want, offsets, [n for _, n in ranges], lead, silence)
        assert all(np.array_equal(a, b) for a, b in zip(got, plain))
        d_got = v.labels_trials_torch(d_wav, ranges, lead=lead, silence=silence, return_energy=True, normalize=flags)
        assert all(np.array_equal(a.cpu().numpy(), np.asarray(b, dtype=a.cpu().numpy().dtype)) for a, b in zip(d_got, plain))
    return audio, peaks, offsets


def test_peak_only_inside_the_dropped_tail(vad, tables):
    wav = _noise(5000, 1)
    wav[1000 + 1200 - 10] = 9000                                                    # among the last `lead` samples of the cut
    audio, peaks, _ = _check(vad, wav, [(1000, 1200)], LEAD, True, tables)
    assert peaks[0] == 9000 and ref.peak(audio) < 200                               # it set the gain and is not in the trial


@pytest.mark.parametrize("value,peak", [(-32768, 32768), (32767, 32767), (0, 0), (1, 1), (-1, 1), (2, 2), (3, 3), (17, 17)])
def test_extreme_peaks(vad, tables, value, peak):
    amp = min(abs(value), 40)
    wav = _noise(4000, 2, amp) if amp else np.zeros(4000, np.int16)
    wav[700] = value
    audio, peaks, _ = _check(vad, wav, [(500, 1000)], LEAD, True, tables)
    assert peaks[0] == peak
    if peak == 0:
        assert not audio.any()
    if peak == 1:                                                                   # three values in, three out; floor rounds -1 further than 1
        lo, mid, hi = np.unique(audio).tolist()
        assert mid == 0 and lo < 0 < hi < -lo and audio[LEAD + 200] == (hi if value > 0 else lo)


def test_a_loud_silence_trial_between_quiet_neighbours(vad, tables):
    wav = _noise(9000, 3)
    wav[3000:6000] = _noise(3000, 4, 20000)
    ranges, silence = [(500, 2000), (3200, 2400), (6500, 2000)], [False, True, False]
    audio, peaks, off = _check(vad, wav, ranges, LEAD, True, tables, silence=silence)
    assert peaks[1] > 100 * max(peaks[0], peaks[2])                                 # reported although the trial is left alone
    assert np.array_equal(audio[off[1]:off[2]], vref.trial_samples(wav, 3200, 2400, LEAD))     # the raw shift
    labels = vad.labels_trials(wav, ranges, lead=LEAD, silence=silence, normalize=True)
    assert len(labels) == 8 + 11 + 8 and not labels[8:19].any()                     # the SILENCE trial's frames


def test_two_overlapping_trials_with_different_peaks(vad, tables):
    wav = _noise(6000, 5)
    wav[1200], wav[2700] = 12000, -3000                                             # the first lies in one trial only
    audio, peaks, off = _check(vad, wav, [(1000, 1500), (2000, 1500)], LEAD, True, tables)
    assert peaks.tolist() == [12000, 3000]
    shared_a = audio[off[0] + LEAD + 1000:off[0] + LEAD + 1200]                     # samples 2000 .. 2200 of the audio, in both
    shared_b = audio[off[1] + LEAD:off[1] + LEAD + 200]
    assert not np.array_equal(shared_a, shared_b)


def test_trials_at_the_end_of_the_audio(vad, tables):
    from dss_amd import _lib
    wav = _noise(5000, 6)
    wav[4990] = 7000
    _, peaks, _ = _check(vad, wav, [(4000, 1000)], LEAD, True, tables)              # ends with the audio: the cut as slicing clamps it
    assert peaks[0] == 7000
    # a cut that would end behind the audio, whose kept samples are all there: the peak is taken over what is there
    audio, peaks, _ = _check(vad, wav, [(4000, 1200)], LEAD, True, tables)
    assert peaks[0] == 7000 and len(audio) == 1200
    with pytest.raises(_lib.DssError, match="lies outside the audio"):
        vad.prepared_audio_trials(wav, [(4000, 1300)], lead=LEAD, normalize=True)


def test_one_window_and_odd_first_samples(vad, tables):
    wav = _noise(9000, 7, 3000)
    for first in (1000, 1001, 1003, 1007):
        _check(vad, wav, [(first, 800)], LEAD, True, tables)
        _check(vad, wav, [(first, 2501)], 0, True, tables)
    _check(vad, wav, [(1, 4000), (2, 4001), (5, 4003), (12, 4098)], LEAD, True, tables)
    # the device buffer itself two bytes off an aligned address
    import torch
    d_wav = torch.from_numpy(wav).cuda()[1:]
    want, want_peaks, _ = ref.prepared_list(wav[1:], [(0, 4200), (7, 800)], LEAD, [True, True], *tables)
    audio, peaks = vad.prepared_audio_trials_torch(d_wav, [(0, 4200), (7, 800)], lead=LEAD, normalize=True, return_peaks=True)
    assert np.array_equal(audio.cpu().numpy(), want) and np.array_equal(peaks.cpu().numpy(), want_peaks)


def test_peaks_at_tile_edges(vad, tables):
    from dss_amd import _lib
    tile = _lib.load().dss_avad_peak_tile()
    assert tile >= 1024
    sizes = (tile - 1, tile, tile + 1, 2 * tile + 1)
    for first in (3000, 3001):                                                      # an aligned and an odd first sample
        wav, ranges, want = _noise(first + sum(sizes) * 4 + 64, 8 + first), [], []
        pos0 = first
        for n in sizes:
            for k, at in enumerate((0, tile - 1, tile, n - 1)):
                if at >= n:
                    continue
                value = 5000 + 100 * len(ranges)
                wav[pos0 + at] = value if k % 2 else -value
                ranges.append((pos0, n))
                want.append(value)
                pos0 += n
        assert len(ranges) >= 13
        _, peaks, _ = _check(vad, wav, ranges, LEAD, True, tables)
        assert peaks.tolist() == want
        for r, w in zip(ranges[:4], want):                                          # and alone
            assert vad.prepared_audio_trials(wav, [r], lead=LEAD, normalize=True, return_peaks=True)[1].tolist() == [w]


def test_a_custom_table_reaches_both_clamps():
    from dss_amd.acoustic_vad import AcousticVadGPU
    table, post = np.full(32769, 2.3), 1.0
    wav = _noise(6000, 9, 30000)
    wav[2000], wav[2001], wav[2002], wav[2003] = 14247, -14247, 14246, -14246       # 2.3 x: 32768.1 / -32768.1 / 32765.8 / -32765.8
    v = AcousticVadGPU()
    try:
        v.set_gain(table, post)
        audio, _, _ = _check(v, wav, [(1000, 3000)], LEAD, True, (table, post))
        assert np.sum(audio == 32767) > 100 and np.sum(audio == -32768) > 100
        assert audio[LEAD + 1000:LEAD + 1004].tolist() == [32767, -32768, 32765, -32766]
        v.set_gain(table, 0.5)                                                      # set again on the same handle
        _check(v, wav, [(1000, 3000)], LEAD, True, (table, 0.5))
    finally:
        v.close()


# ---- 5: orderings and forms -------------------------------------------------------------------------------------------------
def test_list_equals_trial_by_trial_in_any_order(fx, vad):
    wav, b, off = fx["wav"], fx["bounds"], fx["offsets"]
    kw = dict(return_energy=True, normalize=True)
    one = vad.labels_trials(wav, fx["ranges"], lead=fx["lead"], silence=fx["silence"], **kw)
    audio, peaks = vad.prepared_audio_trials(wav, fx["ranges"], lead=fx["lead"], normalize=True, silence=fx["silence"], return_peaks=True)
    again = vad.labels_trials(wav, fx["ranges"], lead=fx["lead"], silence=fx["silence"], **kw)
    assert all(np.array_equal(x, y) for x, y in zip(one, again))                    # a repeated call: the same bits
    assert np.array_equal(vad.prepared_audio_trials(wav, fx["ranges"], lead=fx["lead"], normalize=True, silence=fx["silence"]), audio)
    for k in range(len(fx["ranges"])):
        lab, le, thr = vad.labels_trials(wav, [fx["ranges"][k]], lead=fx["lead"][k], silence=[fx["silence"][k]], **kw)
        assert np.array_equal(lab, one[0][b[k]:b[k + 1]]) and np.array_equal(le, one[1][b[k]:b[k + 1]]) and thr[0] == one[2][k], k
        a, p = vad.prepared_audio_trials(wav, [fx["ranges"][k]], lead=fx["lead"][k], normalize=True, silence=[fx["silence"][k]],
                                         return_peaks=True)
        assert np.array_equal(a, audio[off[k]:off[k + 1]]) and p[0] == peaks[k], k
    perm = np.random.default_rng(11).permutation(len(fx["ranges"]))
    assert not np.array_equal(perm, np.arange(len(perm)))
    pick = lambda xs: [xs[k] for k in perm]
    lab, le, thr = vad.labels_trials(wav, pick(fx["ranges"]), lead=pick(fx["lead"]), silence=pick(fx["silence"]), **kw)
    a, p = vad.prepared_audio_trials(wav, pick(fx["ranges"]), lead=pick(fx["lead"]), normalize=True, silence=pick(fx["silence"]),
                                     return_peaks=True)
    assert np.array_equal(lab, np.concatenate([one[0][b[k]:b[k + 1]] for k in perm]))          # output in LIST order
    assert np.array_equal(le, np.concatenate([one[1][b[k]:b[k + 1]] for k in perm])) and np.array_equal(thr, one[2][perm])
    assert np.array_equal(a, np.concatenate([audio[off[k]:off[k + 1]] for k in perm])) and np.array_equal(p, peaks[perm])


def test_device_resident_form_equals_the_host_form(fx, vad):
    import torch
    kw = dict(lead=fx["lead"], silence=fx["silence"], normalize=True)
    host = vad.labels_trials(fx["wav"], fx["ranges"], return_energy=True, **kw)
    h_audio, h_peaks = vad.prepared_audio_trials(fx["wav"], fx["ranges"], return_peaks=True, **kw)
    d_wav = torch.from_numpy(fx["wav"]).cuda()
    lab, le, thr = vad.labels_trials_torch(d_wav, fx["ranges"], return_energy=True, **kw)
    audio, peaks = vad.prepared_audio_trials_torch(d_wav, fx["ranges"], return_peaks=True, **kw)
    only = vad.prepared_audio_trials_torch(d_wav, fx["ranges"], **kw)
    torch.cuda.synchronize()
    assert lab.dtype == torch.uint8 and np.array_equal(lab.cpu().numpy().astype(bool), host[0])
    assert np.array_equal(le.cpu().numpy(), host[1]) and np.array_equal(thr.cpu().numpy(), host[2])
    assert audio.dtype == torch.int16 and peaks.dtype == torch.int32
    assert np.array_equal(audio.cpu().numpy(), h_audio) and np.array_equal(peaks.cpu().numpy(), h_peaks)
    assert np.array_equal(only.cpu().numpy(), h_audio)
    s = torch.cuda.Stream()                                                         # on a stream of its own, the audio arriving on it
    with torch.cuda.stream(s):
        staged = d_wav.clone()
        lab = vad.labels_trials_torch(staged, fx["ranges"], **kw)
        audio = vad.prepared_audio_trials_torch(staged, fx["ranges"], **kw)
    s.synchronize()
    assert np.array_equal(lab.cpu().numpy().astype(bool), host[0]) and np.array_equal(audio.cpu().numpy(), h_audio)


def test_audio_only_calls_take_trials_shorter_than_a_window(vad, tables):
    from dss_amd import _lib
    wav = _noise(4000, 12, 2000)
    ranges, lead = [(100, 300), (1001, 799), (500, 0), (2000, 256), (3000, 1), (0, 4000)], [256, 0, 0, 256, 0, 17]
    _check(vad, wav, ranges, lead, True, tables, frames=False)
    _check(vad, wav, ranges, lead, [True, False, True, True, False, True], tables, frames=False)
    with pytest.raises(_lib.DssError, match="shorter than one window"):
        vad.labels_trials(wav, ranges, lead=lead, normalize=True)
    assert vad.prepared_audio_trials(wav, []).shape == (0,)
    assert vad.labels_trials(wav, [], normalize=True).shape == (0,)


def test_refusals_reach_the_caller(tables):
    import ctypes as C
    from dss_amd import _lib
    from dss_amd.acoustic_vad import AcousticVadGPU
    v = AcousticVadGPU()
    try:
        L, wav = v._L, _noise(4000, 13)
        first, length, lead = np.array([100], np.int64), np.array([1000], np.int32), np.array([0], np.int32)
        flags, out, labels, le = np.ones(1, np.uint8), np.zeros(1000, np.int16), np.zeros(2, np.uint8), np.zeros(2)

        def call(normalize, labels, le, out):
            ptr = lambda a: a.ctypes.data if a is not None else None
            return L.dss_avad_prepare_trials(v._h, wav.ctypes.data, len(wav), 1, first.ctypes.data, length.ctypes.data,
                                             lead.ctypes.data, None, ptr(normalize), ptr(labels), ptr(le), None, ptr(out), None)
        assert call(flags, None, None, out) == -1 and b"no gain table set" in L.dss_last_error()
        assert call(None, None, None, out) == 0                                     # nothing to normalise: no table needed
        assert np.array_equal(out, wav[100:1100])
        assert call(None, None, le, out) == -1 and b"come with the labels only" in L.dss_last_error()
        assert call(None, None, None, None) == -1 and b"no output asked for" in L.dss_last_error()
        assert call(None, labels, le, None) == 2                                    # the plain labels through the new entry point
        assert np.array_equal(labels.astype(bool), v.labels_trials(wav, [(100, 1000)]))
        bad = tables[0].copy()
        bad[123] = float("nan")
        with pytest.raises(_lib.DssError, match="peak 123 is negative or not finite"):
            v.set_gain(bad)
        with pytest.raises(_lib.DssError, match="post gain"):
            v.set_gain(tables[0], -1.0)
        with pytest.raises(ValueError):
            v.set_gain(tables[0][:100])
        assert call(flags, None, None, out) == -1                                   # a refused table sets nothing
        assert np.array_equal(v.prepared_audio_trials(wav, [(100, 1000)], normalize=True),      # the flag fetches the defaults
                              ref.prepared_list(wav, [(100, 1000)], 0, [True], *tables)[0])
    finally:
        v.close()


# ---- 6: a session -----------------------------------------------------------------------------------------------------------
def test_session_corpus_and_trial_audio(golden, vad, tables):
    from dss_amd import session
    g = golden("session.npz")
    seed, T, c_raw = (int(v) for v in g["recording_seed"])
    rec = synthetic_ecog(seed, T, c_raw)
    fs = int(g["fs"][0])
    all_trials = [tuple(int(v) for v in t) for t in g["trials"]]
    trials = all_trials[1:]                                                          # the first is shorter than one audio window
    labels = ["ba", "ba", "SILENCE", "du", "du"]
    stimuli = ["SILENCE", "ba", "du"]
    wav = synthetic_speech_audio(8500, 16 * T)
    wav[:] = np.trunc(wav * 0.05)                                                    # quiet enough for the gain to matter
    stats = session.normalization_statistics(rec, trials, fs)
    plain = session.session_corpus(rec, wav, trials, labels, stimuli, stats, fs=fs)
    same = session.session_corpus(rec, wav, trials, labels, stimuli, stats, fs=fs, normalize_audio=False)
    assert sorted(plain) == sorted(same) and all(np.array_equal(plain[k], same[k]) for k in plain)
    assert np.array_equal(plain["vad_labels"], session.session_vad_labels(wav, trials, labels, fs))
    corpus = session.session_corpus(rec, wav, trials, labels, stimuli, stats, fs=fs, normalize_audio=True)
    assert sorted(corpus) == ["hga_activity", "trial_ids", "vad_labels"]
    assert np.array_equal(corpus["hga_activity"], plain["hga_activity"]) and np.array_equal(corpus["trial_ids"], plain["trial_ids"])
    # the labels: the pinned plain kernel on the restatement's prepared audio
    ranges = session.trial_audio_ranges(trials, fs, 16000, len(wav))
    silence = [s == "SILENCE" for s in labels]
    want_audio, _, offsets = ref.prepared_list(wav, ranges, LEAD, [not s for s in silence], *tables)
    want = _plain_on_prepared(vad, want_audio, offsets, [n for _, n in ranges], LEAD, silence)[0]
    assert corpus["vad_labels"].dtype == bool and np.array_equal(corpus["vad_labels"], want)
    assert np.array_equal(corpus["vad_labels"], session.session_vad_labels(wav, trials, labels, fs, normalize=True))
    # ... and the restatement's own vote, away from its thresholds
    pos = 0
    for k, (off, (_, n)) in enumerate(zip(offsets, ranges)):
        le = vref.log_energy(want_audio[off:off + n], vad.window_fn, vad.mel)
        lab, thr, _ = vref.vote(le)
        if silence[k]:
            lab[:] = False
        skip = vref.near_threshold(le, thr, 5, 1e-6)
        assert np.array_equal(corpus["vad_labels"][pos:pos + len(le)][~skip], lab[~skip]), k
        pos += len(le)
    assert pos == len(corpus["vad_labels"])
    # what the feature encoder is given, every trial of the session, the short one too
    all_labels = ["du"] + labels
    audio, off = session.session_trial_audio(wav, all_trials, all_labels, fs, 16000)
    all_ranges = session.trial_audio_ranges(all_trials, fs, 16000, len(wav))
    want_audio, _, want_off = ref.prepared_list(wav, all_ranges, LEAD, [s != "SILENCE" for s in all_labels], *tables)
    assert audio.dtype == np.int16 and np.array_equal(audio, want_audio) and np.array_equal(off, want_off)
    louder, _ = session.session_trial_audio(wav, all_trials, all_labels, fs, 16000, norm_db=-1.0)
    assert np.array_equal(louder, ref.prepared_list(wav, all_ranges, LEAD, [s != "SILENCE" for s in all_labels], tables[0], ref.post_gain(-1.0))[0])
