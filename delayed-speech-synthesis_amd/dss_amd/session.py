"""A whole recording session's features and its normalization file, on the GPU.

What the reference does on the CPU before its online decoder can start:

  * ``baseline_offline.py:45-60``: for every trial of a baseline recording a fresh ``HighGammaExtractor``
    (``prepare_corpus.get_feature_extractor``, prepare_corpus.py:147-176) extracts ``ecog[start : stop + 0.04 * fs]``; the
    frames are concatenated and ``normalization.npy = vstack([mean, std])`` is written, which ``decode_online.py:84-95`` and
    ``dss_amd.replay --normalization`` read.
  * ``prepare_corpus.py:42-52,179-199``: the same loop for the training corpus and the per-day z-scores.

Here the recording crosses the bus once and all trials run in one launch (``HgaExtractorGPU.extract_trials``); the frames,
and with them the statistics, are bit-identical to the reference chain.  Parsing the ``.mat`` files stays with the user:
``recording`` is ``BCI2000MatFile.signals()``, ``trials`` the ``(start, stop)`` pairs of ``trial_indices()``.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from . import electrodes
from .hga import HgaExtractorGPU, column_stats

N_GRID_CHANNELS = 128


def offline_frontend(bad_channels: Sequence[int] = electrodes.BAD_CHANNELS):
    """(src_col, grid_of, comp_lists) of get_feature_extractor's pre-transforms (prepare_corpus.py:152-157):
    SelectElectrodesFromBothGrids -> CommonAverageReferencing, 128 output channels, no speech-area selection."""
    cols = np.asarray(electrodes.GRID_COLUMNS, dtype=np.int64)
    grid_of = np.array([next(g for g, (lo, hi) in enumerate(electrodes.GRIDS_ONE_BASED) if lo <= k + 1 <= hi)
                        for k in range(len(cols))])
    bad0 = {b - 1 for b in bad_channels}
    comp_lists = [cols[[k for k in range(lo - 1, hi) if k not in bad0]] for lo, hi in electrodes.GRIDS_ONE_BASED]
    return cols, grid_of, comp_lists


def offline_patches(bad_channels: Sequence[int], contaminated_channels: Sequence[int]):
    """The patches of get_feature_extractor's BadChannelCorrection (prepare_corpus.py:163-170): bad + contaminated channels
    (one-based), the two 8 x 8 grids flipped top to bottom, layout 1..128."""
    speech_grid = np.flip(np.arange(64, dtype=np.int16).reshape((8, 8)) + 1, axis=0)
    motor_grid = np.flip(np.arange(64, dtype=np.int16).reshape((8, 8)) + 65, axis=0)
    corrected = list(bad_channels) + list(contaminated_channels)
    return electrodes.neighbour_patches(corrected, [speech_grid, motor_grid], np.arange(N_GRID_CHANNELS) + 1)


def trial_ranges(trials, fs: int = 1000):
    """[(start, stop)] -> [(start, length)] with baseline_offline.py:49's tail: rows start .. int(stop + 0.04 * fs)."""
    return [(int(start), int(stop + (0.04 * fs)) - int(start)) for start, stop in trials]


def session_extractor(n_raw_columns: int, fs: int = 1000, bad_channels: Optional[Sequence[int]] = None,
                      contaminated_channels: Optional[Sequence[int]] = None) -> HgaExtractorGPU:
    """prepare_corpus.get_feature_extractor as one GPU extractor for trial lists.  ``bad_channels`` are the recording's
    (``BCI2000MatFile.bad_channels()``); as in the reference they matter only together with ``contaminated_channels`` (the
    referencing always leaves out 19, 38, 48, 52: prepare_corpus.py:156)."""
    ex = HgaExtractorGPU(1, N_GRID_CHANNELS, fs=fs)
    ex.set_frontend(int(n_raw_columns), *offline_frontend())
    if contaminated_channels is not None:
        ex.set_patches(offline_patches(list(bad_channels or []), list(contaminated_channels)))
    return ex


def session_features(recording: np.ndarray, trials, fs: int = 1000, bad_channels: Optional[Sequence[int]] = None,
                     contaminated_channels: Optional[Sequence[int]] = None) -> np.ndarray:
    """np.concatenate of every trial's frames (baseline_offline.py:46-53, prepare_corpus.py:42-52): (sum W_i, 128) float64."""
    rec = np.ascontiguousarray(recording, dtype=np.float64)
    ex = session_extractor(rec.shape[1], fs, bad_channels, contaminated_channels)
    try:
        return ex.extract_trials(rec, trial_ranges(trials, fs))
    finally:
        ex.close()


def normalization_statistics(recording: np.ndarray, trials, fs: int = 1000, bad_channels: Optional[Sequence[int]] = None,
                             contaminated_channels: Optional[Sequence[int]] = None) -> np.ndarray:
    """(2, 128) float64 = vstack([mean, std]) over all trials' frames (baseline_offline.py:52-60)."""
    return column_stats(session_features(recording, trials, fs, bad_channels, contaminated_channels))


def save_normalization(path, stats: np.ndarray) -> None:
    """Write what ``np.save(path, np.vstack([mean, std]))`` writes (baseline_offline.py:57-60)."""
    stats = np.asarray(stats, dtype=np.float64)
    if stats.ndim != 2 or stats.shape[0] != 2:
        raise ValueError("statistics must be (2, n_channels): mean row, std row")
    np.save(path, np.vstack([stats[0], stats[1]]))
