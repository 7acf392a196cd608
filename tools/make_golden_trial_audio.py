#!/usr/bin/env python3
"""Generate tests/golden/trial_audio.npz: the trial audio as prepare_corpus.py prepares it, and the reference's own
EnergyBasedVad on it (development machine only: needs the reference tree and Python's ``audioop``).  Run from the repository
root:   python tools/make_golden_trial_audio.py

local/common.py is imported as it lies through oracle/make_golden.py's import_reference_common() (h5py placeholder, asserted
untouched; scipy.hanning bound to numpy.hanning when scipy no longer has it, as tools/make_golden_acoustic_vad.py binds it).
Per trial, as prepare_corpus.get_vad_labels / get_lpc_coefficients do (prepare_corpus.py:58-69, 84-100):

  1. the cut wav[first : first + asked];
  2. unless the trial is a SILENCE trial, pydub's ``effects.normalize(segment).apply_gain(-3.0)`` spelled out as the calls
     pydub makes into Python's own C module: ``audioop.max`` for the peak, ``audioop.mul`` with the factor of that peak, and
     ``audioop.mul`` with the -3 dB factor.  pydub itself is not installed: the two FACTORS are a reading of its wrapper
     (tests/golden/TRIAL_AUDIO.md says which lines, and the check to run once it is); the multiplications are audioop's;
  3. the 16 ms shift: 256 zeros in front, the last 256 samples dropped;
  4. the reference's EnergyBasedVad().from_wav on that array.

Stored: peaks, the two factors, a SHA-256 of every prepared trial (not the audio), log energies, thresholds, labels, frame
counts, and the labels of the same trials WITHOUT step 2.  Provenance row in tests/golden/TRIAL_AUDIO.md.
"""
import audioop
import importlib.util
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "oracle", "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)                      # puts the package on sys.path

SEED, N_LOUD, FS = 7109, 400000, 16000
ZERO = (200000, 215000)                           # samples of the seeded audio set to digital silence
QUIET = 0.02                                      # the second half of the buffer: the first at 2 % amplitude
LEAD = 256                                        # int(0.016 * 16000), prepare_corpus.py:68
HEADROOM_DB, NORM_DB = 0.1, -3.0                  # effects.normalize's default headroom; prepare_corpus's normalization_factor
Q = N_LOUD                                        # first sample of the quiet copy
# (first sample, samples asked for, silence stimulus): wav[first : first + asked] with Python's clamping at the end
TRIALS = [(30000, 800, False),                    # exactly one window
          (52000, 960, False),                    # two frames
          (60000, 40640, False),                  # 2.5 s + 40 ms
          (101000, 64640, False),                 # 4 s + 40 ms
          (149000, 24000, False),                # overlaps the 4 s trial
          (160001, 30000, False),                 # overlaps the previous trial; odd first sample
          (230000, 33000, True),                  # a SILENCE trial with speech in it: not normalised, labels zero
          (201000, 12000, False),                 # digital silence: peak 0, factor 1
          (Q + 60000, 40640, False),              # the 2.5 s trial at 2 % amplitude: the gain moves a label
          (Q + 101000, 64640, False),             # the 4 s trial at 2 % amplitude
          (Q + 149000, 24000, False),
          (Q + 230000, 33000, True),              # a quiet SILENCE trial
          (Q + 381000, 40640, False)]             # clamped at the end of the audio: 19000 samples are there


def build_audio():
    from dss_amd.synthetic import synthetic_speech_audio
    loud = synthetic_speech_audio(SEED, N_LOUD, FS)
    loud[ZERO[0]:ZERO[1]] = 0
    quiet = np.trunc(loud.astype(np.float64) * QUIET).astype(np.int16)      # towards zero: the room noise becomes digital silence
    return np.concatenate([loud, quiet])


def pydub_normalize(cut):
    """effects.normalize(segment).apply_gain(NORM_DB) on int16 samples -> (samples, peak, factor): the audioop calls pydub makes."""
    data = cut.tobytes()
    peak = audioop.max(data, 2)
    if peak == 0:
        factor = 1.0                              # effects.normalize returns a silent segment as it is
    else:
        target = 32768 * 10 ** (-HEADROOM_DB / 20)
        boost = 20 * math.log(target / peak, 10)
        factor = 10 ** (float(boost) / 20)
        data = audioop.mul(data, 2, factor)
    data = audioop.mul(data, 2, 10 ** (float(NORM_DB) / 20))
    return np.frombuffer(data, dtype=np.int16).copy(), peak, factor


def main():
    import scipy
    common, placeholder = mg.import_reference_common()
    bound = not hasattr(scipy, "hanning")
    if bound:
        scipy.hanning = np.hanning
    wav = build_audio()
    pad = np.zeros(int(0.016 * FS), dtype=np.int16)
    assert len(pad) == LEAD

    def label(trial_audio):
        vad = common.EnergyBasedVad()
        lab = np.asarray(vad.from_wav(trial_audio, sampling_rate=FS), dtype=bool)
        le = np.array(vad.mfccs[:, 0], dtype=np.float64)
        return lab, le, vad.vad_energy_threshold + vad.vad_energy_mean_scale * np.sum(le) / len(le)

    desc, peaks, factors, shas, energies, labels, plain, thresholds, counts, gaps = [], [], [], [], [], [], [], [], [], []
    for first, asked, silence in TRIALS:
        cut = wav[first:first + asked]
        peak, factor = int(audioop.max(cut.tobytes(), 2)), 1.0
        prepared = cut
        if not silence:
            prepared, peak, factor = pydub_normalize(cut)
        prepared = np.hstack([pad, prepared[:-len(pad)]])
        raw = np.hstack([pad, cut[:-len(pad)]])
        lab, le, thr = label(prepared)
        lab_plain, _, _ = label(raw)
        if silence:
            assert np.array_equal(prepared, raw) and lab.any()
            lab, lab_plain = np.zeros_like(lab), np.zeros_like(lab_plain)
        desc.append((first, len(prepared), len(pad), int(silence)))
        peaks.append(peak); factors.append(factor); shas.append(np.frombuffer(bytes.fromhex(mg.sha(prepared)), dtype=np.uint8))
        energies.append(le); labels.append(lab); plain.append(lab_plain); thresholds.append(thr); counts.append(len(lab))
        gaps.append(float(np.min(np.abs(le - thr))))
    assert desc[-1][1] == len(wav) - TRIALS[-1][0] < TRIALS[-1][1]                  # the clamped trial
    assert min(gaps) >= 0.8, gaps                 # no frame near its trial's threshold: labels are comparable frame by frame
    moved = [int(np.sum(a != b)) for a, b in zip(labels, plain)]
    quiet_moved = [m for (first, _, _), m in zip(TRIALS, moved) if first >= Q]
    assert any(quiet_moved), moved                # the gain is not label-neutral: a quiet trial's labels differ un-normalised
    assert peaks[7] == 0 and factors[7] == 1.0
    if placeholder is not None:
        assert not placeholder.touched, placeholder.touched
    out = {
        "provenance": np.array("cut, audioop.max / audioop.mul twice (Python %s's own audioop: the calls pydub's effects.normalize and "
                               "apply_gain make; pydub itself not installed, its two factors restated from its wrapper), 16 ms shift, "
                               "then the reference classes (local/common.py imported as it lies: EnergyBasedVad().from_wav per trial); "
                               "h5py placeholder untouched; " % ".".join(str(v) for v in __import__("sys").version_info[:3])
                               + ("scipy.hanning bound to numpy.hanning (scipy %s no longer has it)" % scipy.__version__
                                  if bound else "scipy.hanning as installed")),
        "audio_seed": np.array([SEED, N_LOUD, FS, ZERO[0], ZERO[1]], dtype=np.int64),
        "quiet_scale": np.array(QUIET),
        "audio_sha": np.frombuffer(bytes.fromhex(mg.sha(wav)), dtype=np.uint8),
        "trials_asked": np.array([(a, b) for a, b, _ in TRIALS], dtype=np.int64),
        "trials": np.array(desc, dtype=np.int64),             # first sample, length, leading zeros, silence
        "peaks": np.array(peaks, dtype=np.int32),
        "factors": np.array(factors, dtype=np.float64),       # effects.normalize's factor of each trial's peak (1 where none is applied)
        "post_gain": np.array(10 ** (float(NORM_DB) / 20)),
        "headroom_db": np.array(HEADROOM_DB),
        "prepared_sha": np.stack(shas),
        "frame_counts": np.array(counts, dtype=np.int32),
        "log_energy": np.concatenate(energies),
        "thresholds": np.array(thresholds, dtype=np.float64),
        "labels": np.concatenate(labels),
        "labels_plain": np.concatenate(plain),                # the same trials without the loudness step
    }
    path = os.path.join(mg.GOLD, "trial_audio.npz")
    np.savez_compressed(path, **out)
    le_all = out["log_energy"]
    print("trial_audio: frames per trial", counts, "voiced", int(out["labels"].sum()), "of", len(le_all), os.path.getsize(path), "bytes")
    print("  peaks", peaks)
    print("  labels moved by the loudness step, per trial:", moved)
    print("  smallest |log energy - threshold| per trial:", ["%.3g" % g for g in gaps])
    print("  log energy range", le_all.min(), le_all.max(), "audio sha256", mg.sha(wav))


if __name__ == "__main__":
    main()
