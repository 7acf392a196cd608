#!/usr/bin/env python3
"""Generate tests/golden/gate_cases.npz from the REFERENCE's own classes (development machine only: needs the reference
tree).  Run from the repository root:   python tools/make_golden_gate_cases.py

local/common.py is imported as it lies through oracle/make_golden.py's import_reference_common() (h5py placeholder, asserted
untouched).  Every stream of every case of tests/gate_cases.py runs through VoiceActivityDetectionSmoothing (with the case's
threshold) + SpeechSegmentHistory, chained as FilterSpeechSegments.process chains them (local/units.py:436-447), push by push.

A segment's rows are float32 copies of input frames, so the fixture stores WHICH frames, not their values.  The classes run
twice per stream:
  1. on frames whose every value is the frame's index + 1: a row of a segment then names the input frame it copies, and 0
     names a row of the initially zeroed rings (stored as index -1);
  2. on the case's real frames (tests/gate_cases.py ``frames``): every segment must equal frames.astype(float32)[index], with
     zeros at -1, bit for bit -- asserted here, so that the indices stand for what the classes return on the real data.
Only arrays are written: labels, push sizes, speech frames per push, each segment's stream, push and length, the row indices.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "oracle", "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)                      # puts the package on sys.path
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gate_cases as gc  # noqa: E402


def run_reference(common, c, frames, labels, sizes):
    """-> (speech frames per push, [(push, segment rows float32)]) of one stream."""
    smoothing = common.VoiceActivityDetectionSmoothing(nb_features=c.C, context_frames=c.smoothing_context,
                                                       proportion_threshold=c.threshold)
    history = common.SpeechSegmentHistory(nb_features=c.C, buffer_size=c.N, context=c.context)
    speech, segments, at = [], [], 0
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):       # the casts the ``values`` case is there for
        for k, W in enumerate(sizes.tolist()):
            data, smoothed = smoothing.insert(frames[at:at + W], labels[at:at + W].astype(np.int64))
            for seg in history.insert(data, smoothed):
                seg = np.asarray(seg)
                assert seg.dtype == np.float32 and seg.ndim == 2 and seg.shape[1] == c.C
                segments.append((k, seg))
            speech.append(int(np.count_nonzero(smoothed)))
            at += W
    return speech, segments


def main():
    common, placeholder = mg.import_reference_common()
    out = {}
    n_rows = 0
    for c in gc.CASES:
        sizes = gc.sizes(c.name)
        T = int(sizes.sum())
        all_labels, all_speech, seg_stream, seg_push, seg_len, rows = [], [], [], [], [], []
        for s in range(c.S):
            labels, frames = gc.labels(c.name, s), gc.frames(c.name, s)
            own_index = np.repeat(np.arange(1.0, T + 1.0)[:, None], c.C, axis=1)
            speech_i, segs_i = run_reference(common, c, own_index, labels, sizes)
            speech, segs = run_reference(common, c, frames, labels, sizes)
            assert speech == speech_i and [k for k, _ in segs] == [k for k, _ in segs_i], (c.name, s)
            for (k, seg_i), (_, seg) in zip(segs_i, segs):
                assert np.all(seg_i == seg_i[:, :1]) and np.all(seg_i == np.rint(seg_i)), (c.name, s, k)
                index = seg_i[:, 0].astype(np.int32) - 1
                want = gc.rows_from(frames, index)
                assert seg.shape == want.shape and np.array_equal(gc.bits(seg), gc.bits(want)), (c.name, s, k)
                seg_stream.append(s); seg_push.append(k); seg_len.append(len(index)); rows.append(index)
            all_labels.append(labels); all_speech.append(speech)
        out[f"{c.name}_sizes"] = np.asarray(sizes, dtype=np.int32)
        out[f"{c.name}_labels"] = np.stack(all_labels).astype(np.int8)
        out[f"{c.name}_speech"] = np.array(all_speech, dtype=np.int32)
        out[f"{c.name}_seg_stream"] = np.array(seg_stream, dtype=np.int32)
        out[f"{c.name}_seg_push"] = np.array(seg_push, dtype=np.int32)
        out[f"{c.name}_seg_len"] = np.array(seg_len, dtype=np.int32)
        out[f"{c.name}_rows"] = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
        n_rows += int(sum(seg_len))
        print("  %-14s %3d streams %4d frames %4d segments, lengths %s" % (
            c.name, c.S, T, len(seg_len), (min(seg_len), max(seg_len)) if seg_len else "-"))
    if placeholder is not None:
        assert not placeholder.touched, placeholder.touched
    out["names"] = np.array(gc.NAMES)
    out["provenance"] = np.array(
        "reference classes (local/common.py imported as it lies: VoiceActivityDetectionSmoothing(nb_features, context_frames, "
        "proportion_threshold) + SpeechSegmentHistory(nb_features, buffer_size, context), chained push by push as "
        "FilterSpeechSegments.process chains them); h5py placeholder untouched; rows = index of the input frame a segment's row "
        "copies (-1: zeroed ring), from a run on frames holding their own index + 1, asserted bit for bit against a second run on "
        "the seeded frames of tests/gate_cases.py")
    path = os.path.join(mg.GOLD, "gate_cases.npz")
    np.savez_compressed(path, **out)
    print("gate_cases:", len(gc.CASES), "cases,", n_rows, "segment rows,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
