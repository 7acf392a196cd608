#!/usr/bin/env python3
"""Generate tests/golden/acoustic_vad.npz from the REFERENCE's own classes (development machine only: needs the reference
tree).  Run from the repository root:   python tools/make_golden_acoustic_vad.py

local/common.py is imported as it lies through oracle/make_golden.py's import_reference_common() (h5py placeholder, asserted
untouched).  Per trial the reference's own EnergyBasedVad().from_wav runs on the trial's audio, cut and shifted by 16 ms as
prepare_corpus.get_vad_labels does (prepare_corpus.py:84-93), WITHOUT its pydub loudness normalisation (not installed, and
outside the package's contract); MelFilterBank(401, 40, 16000) gives the matrix.

One binding is made: from_wav calls scipy.hanning, which scipy >= 1.15 no longer has.  It was numpy's hanning re-exported
(scipy's removal notice: "use numpy.hanning instead"), so scipy.hanning = numpy.hanning is set when the attribute is missing,
and the provenance field records it.  Only arrays are written; provenance row in tests/golden/ACOUSTIC_VAD.md.
"""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "oracle", "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)                      # puts the package on sys.path

SEED, N_AUDIO, FS = 7109, 400000, 16000
ZERO = (200000, 215000)                           # samples of the seeded audio set to digital silence
LEAD = 256                                        # int(0.016 * 16000), prepare_corpus.py:92
# (first sample, samples asked for, silence stimulus): audio[first : first + asked] with Python's clamping at the end
TRIALS = [(30000, 800, False),                    # exactly one window: one frame, den = 0 or 1
          (52000, 960, False),                    # two frames: den is 1 or 2 everywhere
          (60000, 40640, False),                  # 2.5 s + 40 ms
          (101000, 64640, False),                 # 4 s + 40 ms
          (150000, 24000, False),                 # overlaps the 4 s trial's samples 150000 .. 165640
          (160000, 30000, False),                 # overlaps the previous trial
          (380000, 40640, False),                 # clamped at the end of the audio: 20000 samples are there
          (230000, 33000, True),                  # a SILENCE trial with speech in it: labels zero whatever the energies say
          (201000, 12000, False)]                 # digital silence: log(1e-7) in every band


def main():
    import scipy
    from dss_amd.synthetic import synthetic_speech_audio
    common, placeholder = mg.import_reference_common()
    bound = not hasattr(scipy, "hanning")
    if bound:
        scipy.hanning = np.hanning
    wav = synthetic_speech_audio(SEED, N_AUDIO, FS)
    wav[ZERO[0]:ZERO[1]] = 0
    desc, energies, labels, thresholds, counts = [], [], [], [], []
    for first, asked, silence in TRIALS:
        trial_audio = wav[first:first + asked]
        pad = np.zeros(int(0.016 * FS), dtype=np.int16)
        trial_audio = np.hstack([pad, trial_audio[:-len(pad)]])
        vad = common.EnergyBasedVad()
        lab = vad.from_wav(trial_audio, sampling_rate=FS)
        le = np.array(vad.mfccs[:, 0], dtype=np.float64)
        thresholds.append(vad.vad_energy_threshold + vad.vad_energy_mean_scale * np.sum(le) / len(le))
        if silence:
            assert np.asarray(lab).any(), "the SILENCE trial must hold speech for its zero labels to mean something"
            lab = np.zeros_like(lab)
        desc.append((first, len(trial_audio), len(pad), int(silence)))
        energies.append(le)
        labels.append(np.asarray(lab, dtype=bool))
        counts.append(len(lab))
    mfb = common.MelFilterBank(401, 40, FS)
    le_all = np.concatenate(energies)
    gaps = [float(np.min(np.abs(e - t))) for e, t in zip(energies, thresholds)]
    assert desc[6][1] == N_AUDIO - TRIALS[6][0] and counts[0] == 1 and counts[1] == 2
    assert np.concatenate(labels).any() and not np.concatenate(labels).all()
    assert min(gaps) >= 0.8, gaps                 # no frame near its trial's threshold: labels are comparable frame by frame
    assert np.all(energies[8] == energies[8][0]) and not labels[8].any()      # digital silence: log(1e-7) in every band
    out = {
        "provenance": np.array("reference classes (local/common.py imported as it lies: EnergyBasedVad().from_wav per trial, "
                               "MelFilterBank(401, 40, 16000)); h5py placeholder untouched; "
                               + ("scipy.hanning bound to numpy.hanning (scipy %s no longer has it); " % scipy.__version__
                                  if bound else "scipy.hanning as installed; ")
                               + "no pydub loudness normalisation"),
        "audio_seed": np.array([SEED, N_AUDIO, FS, ZERO[0], ZERO[1]], dtype=np.int64),
        "audio_sha": np.frombuffer(bytes.fromhex(mg.sha(wav)), dtype=np.uint8),
        "trials_asked": np.array([(a, b) for a, b, _ in TRIALS], dtype=np.int64),
        "trials": np.array(desc, dtype=np.int64),             # first sample, length, leading zeros, silence
        "frame_counts": np.array(counts, dtype=np.int32),
        "log_energy": le_all,
        "thresholds": np.array(thresholds, dtype=np.float64),
        "labels": np.concatenate(labels),
        "mel": np.ascontiguousarray(mfb.melMatrix, dtype=np.float64),
        "window": np.asarray(scipy.hanning(800), dtype=np.float64),
    }
    if placeholder is not None:
        assert not placeholder.touched, placeholder.touched
    np.savez_compressed(os.path.join(mg.GOLD, "acoustic_vad.npz"), **out)
    print("acoustic_vad: frames per trial", counts, "voiced", int(out["labels"].sum()), "of", len(le_all))
    print("  smallest |log energy - threshold| per trial:", ["%.3g" % g for g in gaps])
    print("  log energy range", le_all.min(), le_all.max(), "audio sha256", mg.sha(wav))


if __name__ == "__main__":
    main()
