"""Host side of the progressive (frame-by-frame) segment delivery that needs no GPU: the new C ABI entry points are declared and
exported, and the bookkeeping that turns frame counters into pieces of audio (dss_amd.segment_queue.progress_chunks)."""
import importlib
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dss_host_alloc_fine", "dss_progress_read", "dss_lpcnet_batch_synthesize_ragged_progress_dev")


def _chunks():
    return importlib.import_module("dss_amd.segment_queue").progress_chunks


def test_progress_entry_points_are_declared_and_exported():
    from dss_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dss_hip.h")).read(), flags=re.S)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name


def test_counters_become_contiguous_pieces_with_one_last_each():
    progress_chunks = _chunks()
    lengths = [5, 3]
    sent = [0, 0]
    assert progress_chunks(lengths, sent, [0, 0]) == []                         # nothing there yet
    assert progress_chunks(lengths, sent, [1, 0]) == [(0, 0, 1, False)]
    assert progress_chunks(lengths, sent, [1, 0]) == []                         # unchanged counters: nothing new
    assert progress_chunks(lengths, sent, [4, 3]) == [(0, 1, 4, False), (1, 0, 3, True)]   # a jump of 3 frames is one piece
    assert sent == [4, -1]
    assert progress_chunks(lengths, sent, [5, 3]) == [(0, 4, 5, True)]
    assert progress_chunks(lengths, sent, [5, 3]) == [] and progress_chunks(lengths, sent, [5, 3], retired=True) == []


def test_zero_length_segment_gives_one_empty_last_piece():
    progress_chunks = _chunks()
    sent = [0, 0]
    assert progress_chunks([0, 2], sent, [0, 0]) == [(0, 0, 0, True)]
    assert progress_chunks([0, 2], sent, [0, 0]) == []
    assert progress_chunks([0, 2], sent, [0, 0], retired=True) == [(1, 0, 2, True)]
    sent = [0]
    assert progress_chunks([0], sent, [0], retired=True) == [(0, 0, 0, True)]


def test_retire_after_a_partial_read_sends_the_rest():
    progress_chunks = _chunks()
    sent = [0, 0, 0]
    assert progress_chunks([6, 4, 2], sent, [2, 0, 2]) == [(0, 0, 2, False), (2, 0, 2, True)]
    assert progress_chunks([6, 4, 2], sent, None, retired=True) == [(0, 2, 6, True), (1, 0, 4, True)]
    assert sent == [-1, -1, -1]


def test_pieces_concatenate_to_the_segment_under_any_counter_sequence():
    """Random non-decreasing counter sequences (steps of 0 to several frames, retire at any point): every row's pieces start
    where the previous one ended, cover [0, length) exactly and end with one last piece."""
    progress_chunks = _chunks()
    rng = np.random.default_rng(3)
    for _ in range(200):
        lengths = [int(x) for x in rng.integers(0, 12, int(rng.integers(1, 6)))]
        sent = [0] * len(lengths)
        c = np.zeros(len(lengths), dtype=np.int32)
        got = {k: [] for k in range(len(lengths))}
        for step in range(int(rng.integers(0, 8))):
            c = np.minimum(c + rng.integers(0, 4, len(lengths)), lengths).astype(np.int32)
            for k, f0, f1, last in progress_chunks(lengths, sent, c):
                got[k].append((f0, f1, last))
        for k, f0, f1, last in progress_chunks(lengths, sent, c, retired=True):
            got[k].append((f0, f1, last))
        for k, n in enumerate(lengths):
            p = got[k]
            assert p and p[0][0] == 0 and p[-1][1] == n and p[-1][2], (lengths, p)
            assert [x[2] for x in p].count(True) == 1
            assert all(a[1] == b[0] for a, b in zip(p, p[1:])) and all(f1 > f0 for f0, f1, _ in p[:-1] or [])
