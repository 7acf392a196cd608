#!/usr/bin/env python3
"""Generate tests/golden/session.npz from the REFERENCE's own classes (development machine only: needs the reference tree
that `make -C oracle ref` compiles from).  Run from the repository root:   python tools/make_golden_session.py

The chain is prepare_corpus.get_feature_extractor's (prepare_corpus.py:147-176), built from the reference's objects:
SelectElectrodesFromBothGrids -> CommonAverageReferencing([19, 38, 48, 52]) -> HighGammaExtractor (a FRESH one per trial, the
whole trial as one chunk) -> BadChannelCorrection(bad + contaminated), then np.concatenate / np.mean / np.std as
baseline_offline.py:45-60 runs them.  local/common.py is imported as it lies (with oracle/make_golden.py's h5py placeholder,
asserted untouched; provenance row in tests/golden/SESSION.md); local/units.py cannot be imported here, so its extract_features is driven by oracle/make_golden.py's
RefExtractor around the reference's compiled hga_optimized module.  Only arrays are written.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "oracle", "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)                      # puts the package and oracle/_ref on sys.path
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, REF_DIR)                       # the reference's compiled hga_optimized, not the package's drop-in of that name

SEED, T, C_RAW, FS = 6000, 3100, 129, 1000
BAD = [19, 38, 48, 52]                            # BCI2000MatFile.bad_channels() of the reference's recordings
CONTAMINATED = [1, 28, 100, 101, 128]             # a speech-grid corner (3 neighbours), inner channels, motor grid, its corner
# (start, stop) as BCI2000MatFile.trial_indices() yields them; rows start .. stop + 40 are extracted (baseline_offline.py:49)
TRIALS = [(100, 105),       # 45 rows: CASE 2 of the frame buffer, one zero-padded frame
          (200, 210),       # exactly 50 rows: CASE 1, one frame
          (300, 1617),      # 1357 rows: 131 windows, more than the kernel's window table
          (1500, 1793),     # 333 rows, overlaps the previous trial's rows 1500 .. 1656
          (1700, 2287),     # 627 rows, overlaps the previous trial
          (2400, 2977)]     # 617 rows


def main():
    from dss_amd.synthetic import synthetic_ecog
    import hga_optimized
    assert os.path.dirname(os.path.abspath(hga_optimized.__file__)) == REF_DIR, hga_optimized.__file__
    common, placeholder = mg.import_reference_common()
    hg, fh, zi_hg, zi_fh = mg.design()
    speech_grid = np.flip(np.arange(64, dtype=np.int16).reshape((8, 8)) + 1, axis=0)
    motor_grid = np.flip(np.arange(64, dtype=np.int16).reshape((8, 8)) + 65, axis=0)
    layout = np.arange(128) + 1
    select = common.SelectElectrodesFromBothGrids()
    car = common.CommonAverageReferencing(exclude_channels=[19, 38, 48, 52], grids=[speech_grid, motor_grid], layout=layout)
    correction = common.BadChannelCorrection(bad_channels=BAD + CONTAMINATED, grids=[speech_grid, motor_grid], layout=layout)

    rec = synthetic_ecog(SEED, T, C_RAW)
    plain, corrected = [], []
    for start, stop in TRIALS:
        chunk = rec[start:int(stop + (0.04 * FS)), :]
        frames = mg.RefExtractor(FS, len(select), hg, fh, zi_hg, zi_fh).extract(car(select(chunk)))
        plain.append(frames)
        corrected.append(correction(frames))
    counts = np.array([len(f) for f in plain], dtype=np.int32)
    plain, corrected = np.concatenate(plain), np.concatenate(corrected)
    dst = np.array([int(np.asarray(loc).reshape(-1)[0]) for loc, _ in correction.patches], dtype=np.int32)
    untouched = np.setdiff1d(np.arange(128), dst)
    assert np.array_equal(plain[:, untouched], corrected[:, untouched])      # only the corrected columns are stored twice
    sizes = sorted(len(nb) for _, nb in correction.patches)
    assert sizes[0] == 3 and sizes[-1] == 8 and any(d >= 64 for d in dst), sizes
    out = {
        "provenance": np.array("reference classes (local/common.py imported as it lies, extensions/hga/hga_optimized.pyx compiled "
                               "unmodified, extract_features driven by oracle/make_golden.py RefExtractor); h5py placeholder untouched"),
        "recording_seed": np.array([SEED, T, C_RAW], dtype=np.int64),
        "recording_sha": np.frombuffer(bytes.fromhex(mg.sha(rec)), dtype=np.uint8),
        "fs": np.array([FS], dtype=np.int32),
        "trials": np.array(TRIALS, dtype=np.int64),
        "frame_counts": counts,
        "bad_channels": np.array(BAD, dtype=np.int32),
        "contaminated_channels": np.array(CONTAMINATED, dtype=np.int32),
        "patch_dst": dst,
        "patch_cols": np.concatenate([np.asarray(nb) for _, nb in correction.patches]).astype(np.int32),
        "patch_off": np.concatenate([[0], np.cumsum([len(nb) for _, nb in correction.patches])]).astype(np.int32),
        "frames": plain,                                    # without BadChannelCorrection (contaminated_channels() is None)
        "corrected_columns": corrected[:, dst],             # the patched columns of the chain with it
        "mean_plain": np.mean(plain, axis=0), "std_plain": np.std(plain, axis=0),
        "mean": np.mean(corrected, axis=0), "std": np.std(corrected, axis=0),
    }
    if placeholder is not None:
        assert not placeholder.touched, placeholder.touched
    np.savez(os.path.join(mg.GOLD, "session.npz"), **out)
    print("session:", plain.shape, "frames per trial", counts.tolist(), "neighbours per patch", [len(nb) for _, nb in correction.patches])


if __name__ == "__main__":
    main()
