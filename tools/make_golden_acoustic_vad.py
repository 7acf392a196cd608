#!/usr/bin/env python3
"""Generate tests/golden/acoustic_vad.npz and tests/golden/acoustic_vad_cases.npz from the REFERENCE's own classes (development
machine only: needs the reference tree).  Run from the repository root:   python tools/make_golden_acoustic_vad.py [fixture] [cases]
(both without an argument; ``cases`` alone leaves acoustic_vad.npz as it is -- see ``cases()`` for the second file).

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


def cases():
    """tests/golden/acoustic_vad_cases.npz: the geometry cases of tests/acoustic_vad_cases.py through the reference's own
    EnergyBasedVad.  window_length and frame_shift are attributes of the instance and the sampling rate an argument of from_wav,
    so those three are set as a caller would set them.  The band count is the literal 40 inside from_wav: for the cases with
    another count common.MelFilterBank is bound, for that call, to a wrapper that hands the class the case's count in its place
    (a binding of the same kind as scipy.hanning's).  The mel matrices are not stored; the generator asserts that
    dss_amd.acoustic_vad.mel_filterbank gives the reference's matrix bit for bit at every case, and that no stored frame lies
    within GAP of its trial's threshold."""
    import sys
    import scipy
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import acoustic_vad_cases as vc
    from dss_amd import acoustic_vad
    common, placeholder = mg.import_reference_common()
    bound = not hasattr(scipy, "hanning")
    if bound:
        scipy.hanning = np.hanning
    reference_bank = common.MelFilterBank
    seen = {}

    def bank_with(n_bands):
        def make(spec_size, num_coefficients, sample_rate):
            assert num_coefficients == 40, num_coefficients
            seen["bank"] = reference_bank(spec_size, n_bands, sample_rate)
            return seen["bank"]
        return make

    geometry, trials, counts, energies, thresholds, labels, seeds, shas, wrapped = [], [], [], [], [], [], [], [], []
    gaps = {}
    for c in vc.GEOMETRY:
        wav = vc.audio(c.name)
        common.MelFilterBank = bank_with(c.n_bands)
        try:
            for first, n in vc.trials(c.name):
                vad = common.EnergyBasedVad()
                vad.window_length, vad.frame_shift = c.window_length, c.frame_shift
                lab = np.asarray(vad.from_wav(wav[first:first + n], sampling_rate=c.fs), dtype=bool)
                le = np.array(vad.mfccs[:, 0], dtype=np.float64)
                thr = vad.vad_energy_threshold + vad.vad_energy_mean_scale * np.sum(le) / len(le)
                gap = float(np.min(np.abs(le - thr)))
                assert gap >= vc.GAP, (c.name, first, n, gap)           # move the trial's first sample (vc.FIRST_AT), keep the gap
                gaps[c.name] = min(gap, gaps.get(c.name, np.inf))
                mel = seen["bank"].melMatrix
                assert mel.shape == (c.bins, c.n_bands) and len(le) == (n - c.N) // c.shift + 1
                trials.append((first, n)); counts.append(len(le)); energies.append(le); thresholds.append(thr); labels.append(lab)
        finally:
            common.MelFilterBank = reference_bank
        assert np.array_equal(acoustic_vad.mel_filterbank(c.bins, c.n_bands, c.fs), mel), c.name
        assert int(np.sum(~mel.any(axis=0))) == c.empty, (c.name, int(np.sum(~mel.any(axis=0))))
        assert counts[-4:] == list(vc.TRIAL_FRAMES), (c.name, counts[-4:])
        geometry.append((c.fs, c.N, c.shift, c.bins, c.n_bands))
        seeds.append((vc.audio_seed(c.name), len(wav)))
        shas.append(np.frombuffer(bytes.fromhex(mg.sha(wav)), dtype=np.uint8))
        wrapped.append(c.n_bands != 40)
    if placeholder is not None:
        assert not placeholder.touched, placeholder.touched
    out = {
        "provenance": np.array("reference classes (local/common.py imported as it lies: EnergyBasedVad() per trial with window_length "
                               "and frame_shift set on the instance, from_wav(trial, sampling_rate=fs)); h5py placeholder untouched; "
                               + ("scipy.hanning bound to numpy.hanning (scipy %s no longer has it); " % scipy.__version__
                                  if bound else "scipy.hanning as installed; ")
                               + "common.MelFilterBank bound to a wrapper that replaces from_wav's literal 40 by the case's band "
                               "count, for the cases flagged in band_wrapper; no pydub loudness normalisation; lead 0"),
        "names": np.array(vc.NAMES),
        "geometry": np.array(geometry, dtype=np.int64),               # fs, N, shift, bins, bands
        "band_wrapper": np.array(wrapped, dtype=bool),
        "audio_seed": np.array(seeds, dtype=np.int64),                # seed, samples (at the case's fs)
        "audio_sha": np.stack(shas),
        "trials": np.array(trials, dtype=np.int64),                   # first sample, length; four per case, case after case
        "frame_counts": np.array(counts, dtype=np.int32),
        "log_energy": np.concatenate(energies),
        "thresholds": np.array(thresholds, dtype=np.float64),
        "labels": np.concatenate(labels),
    }
    path = os.path.join(mg.GOLD, "acoustic_vad_cases.npz")
    np.savez_compressed(path, **out)
    le_all = out["log_energy"]
    print("acoustic_vad_cases:", len(vc.GEOMETRY), "cases,", len(le_all), "frames,", int(out["labels"].sum()), "voiced,",
          os.path.getsize(path), "bytes")
    print("  smallest |log energy - threshold| per case:", {k: "%.3g" % v for k, v in gaps.items()})
    print("  log energy range", le_all.min(), le_all.max())


if __name__ == "__main__":
    import sys
    which = sys.argv[1:] or ["fixture", "cases"]
    if "fixture" in which:
        main()
    if "cases" in which:
        cases()
