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

  * ``prepare_corpus.py:78-137,202-234``: the corpus file of a recording -- ``hga_activity`` (the z-scored frames),
    ``vad_labels`` (an ``EnergyBasedVad`` per trial on the session's wav) and ``trial_ids``: ``session_corpus`` below, with
    the labels of all trials in one pass over the audio (``AcousticVadGPU.labels_trials``).  The per-trial loudness
    normalisation through pydub is opt-in (``normalize_audio=True``; by default the audio is labelled as it is handed over);
    its arithmetic is pinned by tests/golden/trial_audio.npz.
  * ``prepare_corpus.py:55-76``: ``lpc_coefficients`` -- ``session_lpc_coefficients`` below (and ``session_corpus`` with
    ``lpc_coefficients=True``): the array ``session_trial_audio`` prepares per trial, through the LPC feature encoder
    (``feature_encoder.LpcFeatureEncoderGPU``) for all trials in one call.  That encoder is this project's statement of the
    published method; parity with xiph's ``LPCFeatureEncoder`` is not pinned.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from . import acoustic_vad, electrodes, hga
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


# ---- the training corpus of one recording (prepare_corpus.py:78-137, 202-234) ------------------------------------------------
def trial_audio_ranges(trials, fs: int = 1000, fs_audio: int = 16000, n_audio: Optional[int] = None):
    """[(start, stop)] in recording rows -> [(first, length)] in audio samples (prepare_corpus.py:84-87):
    ``wav[int(start * fs_audio / fs) : int(stop * fs_audio / fs) + int(0.04 * fs_audio)]``, clamped to ``n_audio`` samples as
    Python's slicing clamps a range that ends behind the file."""
    out = []
    for start, stop in trials:
        a = int(start * fs_audio / fs)
        b = int(stop * fs_audio / fs) + int(0.04 * fs_audio)
        if n_audio is not None:
            a, b = min(a, int(n_audio)), min(b, int(n_audio))
        out.append((a, max(b - a, 0)))
    return out


def session_vad_labels(wav: np.ndarray, trials, stimulus_labels, fs: int = 1000, fs_audio: int = 16000,
                       shift_seconds: float = 0.016, vad: Optional[acoustic_vad.AcousticVadGPU] = None,
                       normalize: bool = False) -> np.ndarray:
    """np.concatenate of every trial's EnergyBasedVad labels (prepare_corpus.get_vad_labels): bool (sum W_i,).  ``wav`` is the
    session's int16 audio.  By default it is labelled AS IT IS; with ``normalize`` every trial whose stimulus label is not
    "SILENCE" is first brought to the reference's loudness (prepare_corpus.py:88-89: pydub's normalize and -3 dB, on the
    device; ``AcousticVadGPU.set_gain``'s defaults unless ``vad`` was given other data).  Every trial is shifted by
    ``shift_seconds`` (zeros in front, the tail dropped, prepare_corpus.py:91-93); trials whose stimulus label is "SILENCE" get
    all-zero labels (prepare_corpus.py:99-100)."""
    wav = np.asarray(wav)
    ranges = trial_audio_ranges(trials, fs, fs_audio, len(wav))
    silence = [label == "SILENCE" for label in stimulus_labels]
    if len(silence) != len(ranges):
        raise ValueError("one stimulus label per trial")
    own = vad is None
    v = acoustic_vad.AcousticVadGPU(fs=fs_audio) if own else vad
    try:
        return v.labels_trials(wav, ranges, lead=int(shift_seconds * fs_audio), silence=silence,
                               normalize=True if normalize else None)
    finally:
        if own:
            v.close()


def session_trial_audio(wav: np.ndarray, trials, stimulus_labels, fs: int = 1000, fs_audio: int = 16000,
                        shift_seconds: float = 0.016, norm_db: float = -3.0,
                        vad: Optional[acoustic_vad.AcousticVadGPU] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Per trial exactly the array prepare_corpus.py:73 hands ``LPCFeatureEncoder.compute_LPC_features``
    (prepare_corpus.py:58-69): the cut, normalised through pydub's two gains unless the stimulus is "SILENCE", shifted by
    ``shift_seconds``.  Returns ``(int16 concatenation, offsets)``: trial i is ``audio[offsets[i] : offsets[i + 1]]``.  A trial
    may be shorter than a VAD window here.  ``norm_db`` is get_lpc_coefficients' ``norm``.  A ``vad`` handed in is left with
    pydub's table and that post gain set (``AcousticVadGPU.set_gain``)."""
    from . import trial_audio
    wav = np.asarray(wav)
    ranges = trial_audio_ranges(trials, fs, fs_audio, len(wav))
    silence = [label == "SILENCE" for label in stimulus_labels]
    if len(silence) != len(ranges):
        raise ValueError("one stimulus label per trial")
    own = vad is None
    v = acoustic_vad.AcousticVadGPU(fs=fs_audio) if own else vad
    try:
        v.set_gain(post=trial_audio.post_gain(norm_db))
        out = v.prepared_audio_trials(wav, ranges, lead=int(shift_seconds * fs_audio), normalize=True, silence=silence)
    finally:
        if own:
            v.close()
    return out, np.concatenate([[0], np.cumsum([n for _, n in ranges], dtype=np.int64)]).astype(np.int64)


def lpc_rows(n_samples: int) -> int:
    """Rows of ``lpc_coefficients`` a trial of ``n_samples`` prepared samples gives: ``features[3:-1]`` of its n // 160 frames
    (prepare_corpus.py:74)."""
    return max(int(n_samples) // 160 - 4, 0)


def session_lpc_coefficients(wav: np.ndarray, trials, stimulus_labels, fs: int = 1000, fs_audio: int = 16000,
                             shift_seconds: float = 0.016, norm_db: float = -3.0) -> np.ndarray:
    """prepare_corpus.get_lpc_coefficients (prepare_corpus.py:55-76): float32 (sum rows_i, 20).  Every trial's audio is
    prepared as ``session_trial_audio`` prepares it and stays on the device; a fresh encoder per trial, all trials in one call
    (``LpcFeatureEncoderGPU.features_trials_torch``); ``features[3:-1]`` of every trial, concatenated.  The encoder is this
    project's statement of the published method; parity with xiph's is not pinned."""
    import torch
    from . import feature_encoder, trial_audio
    wav = np.asarray(wav)
    if wav.dtype != np.int16 or wav.ndim != 1:
        raise ValueError("wav must be a one-dimensional int16 array")
    ranges = trial_audio_ranges(trials, fs, fs_audio, len(wav))
    silence = [label == "SILENCE" for label in stimulus_labels]
    if len(silence) != len(ranges):
        raise ValueError("one stimulus label per trial")
    offsets = np.concatenate([[0], np.cumsum([n for _, n in ranges], dtype=np.int64)]).astype(np.int64)
    v = acoustic_vad.AcousticVadGPU(fs=fs_audio)
    enc = feature_encoder.LpcFeatureEncoderGPU()
    try:
        v.set_gain(post=trial_audio.post_gain(norm_db))
        d_wav = torch.from_numpy(np.ascontiguousarray(wav)).cuda()
        audio = v.prepared_audio_trials_torch(d_wav, ranges, lead=int(shift_seconds * fs_audio), normalize=True, silence=silence)
        feats, fo = enc.features_trials_torch(audio, offsets)
        keep = [feats[int(fo[i]) + 3:int(fo[i + 1]) - 1] for i in range(len(ranges)) if fo[i + 1] - fo[i] > 4]
        out = torch.cat(keep) if keep else feats[:0]
        return out.cpu().numpy()
    finally:
        enc.close()
        v.close()


def trial_ids(trials, stimulus_labels, stimuli, fs: int = 1000) -> np.ndarray:
    """prepare_corpus.get_trial_ids (prepare_corpus.py:118-137): per frame the one-based index of the trial's stimulus in
    ``stimuli``, negated when the trial repeats the stimulus of the trial before it (and positive again on the next
    repetition), int16."""
    stimuli = list(stimuli)
    ids = []
    last = None
    for (start, stop), label in zip(trials, stimulus_labels):
        interval = int(stop + (0.04 * fs)) - start
        num_windows = int(np.floor((interval - 0.04 * fs) / (0.01 * fs)))
        code = stimuli.index(label) + 1
        if last is None or last != code:
            last = code
        else:
            last = code * -1
        ids.append(np.ones(num_windows) * last)
    return np.hstack(ids).astype(np.int16) if ids else np.zeros(0, dtype=np.int16)


def session_corpus(recording: np.ndarray, wav: np.ndarray, trials, stimulus_labels, stimuli, normalization: np.ndarray,
                   fs: int = 1000, fs_audio: int = 16000, bad_channels: Optional[Sequence[int]] = None,
                   contaminated_channels: Optional[Sequence[int]] = None, shift_seconds: float = 0.016,
                   normalize_audio: bool = False, lpc_coefficients: bool = False, norm_db: float = -3.0) -> dict:
    """The arrays prepare_corpus.main stores per recording (prepare_corpus.py:218-234), ready for the user's own
    ``save_data_to_hdf``: ``hga_activity`` = (session_features - mean) / std with ``normalization`` = vstack([mean, std]) of the
    day, ``vad_labels`` (bool), ``trial_ids`` (int16).  Raises ValueError when a trial's frame count differs between the
    features and the labels (a trial clamped at the end of the wav, a sampling-rate ratio that truncates): the reference
    would write misaligned arrays.  With ``lpc_coefficients=True`` the fourth array is added under that key
    (``session_lpc_coefficients``: float32 (N, 20), this project's statement of the encoder, parity with xiph's not pinned;
    ``norm_db`` is get_lpc_coefficients' ``norm``), and a trial whose row count there differs from its feature frames raises
    ValueError too; without the keyword the dict has the three keys only.  By default the wav is labelled as it is handed over; with
    ``normalize_audio`` every non-SILENCE trial gets the reference's pydub loudness normalisation first (on the device), which
    is what prepare_corpus.get_vad_labels labels."""
    trials = [(int(a), int(b)) for a, b in trials]
    stats = np.asarray(normalization, dtype=np.float64)
    if stats.ndim != 2 or stats.shape[0] != 2:
        raise ValueError("normalization must be (2, n_channels): mean row, std row")
    v_window, v_shift = int(fs_audio * 0.05), int(fs_audio * 0.01)
    for k, ((_, n_rows), (_, n_samples)) in enumerate(zip(trial_ranges(trials, fs), trial_audio_ranges(trials, fs, fs_audio, len(wav)))):
        w_hga = hga.trial_frames(n_rows, fs)
        w_vad = acoustic_vad.trial_frames(n_samples, v_window, v_shift)
        if w_hga != w_vad:
            raise ValueError(f"trial {k}: {w_hga} feature frames but {w_vad} label frames")
        if lpc_coefficients and w_hga != lpc_rows(n_samples):
            raise ValueError(f"trial {k}: {w_hga} feature frames but {lpc_rows(n_samples)} rows of LPC coefficients")
    feats = session_features(recording, trials, fs, bad_channels, contaminated_channels)
    if normalize_audio:
        labels = session_vad_labels(wav, trials, stimulus_labels, fs, fs_audio, shift_seconds, normalize=True)
    else:
        labels = session_vad_labels(wav, trials, stimulus_labels, fs, fs_audio, shift_seconds)
    ids = trial_ids(trials, stimulus_labels, stimuli, fs)
    if not (len(feats) == len(labels) == len(ids)):
        raise ValueError(f"misaligned corpus: {len(feats)} feature frames, {len(labels)} labels, {len(ids)} trial ids")
    corpus = dict(hga_activity=(feats - stats[0]) / stats[1], vad_labels=labels, trial_ids=ids)
    if lpc_coefficients:
        lpc = session_lpc_coefficients(wav, trials, stimulus_labels, fs, fs_audio, shift_seconds, norm_db)
        if len(lpc) != len(feats):
            raise ValueError(f"misaligned corpus: {len(feats)} feature frames, {len(lpc)} rows of LPC coefficients")
        corpus["lpc_coefficients"] = lpc
    return corpus
