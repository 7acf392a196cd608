"""Progressive (frame-by-frame) delivery of vocoder PCM to the host: dss_lpcnet_batch_synthesize_ragged_progress_dev and
SegmentSynthesisQueue(progressive=True).  The bytes that reach the host are the whole-segment path's bytes, in order
(local/units.py:531-538,550-552); they only arrive a 10 ms frame at a time, while the kernel runs."""
import ctypes as C
import os
import sys
import threading
import time

import numpy as np
import pytest
import torch

from dss_amd.lpcnet_weights import synthetic_blob, synthetic_features

pytestmark = pytest.mark.gpu
FRAME = 160
DSS_EINVAL = -1


class _Fine:
    """A block of dss_host_alloc_fine memory seen as a numpy array."""

    def __init__(self, L, n, ctype):
        self.L, self.ptr = L, L.dss_host_alloc_fine(n * C.sizeof(ctype))
        assert self.ptr, L.dss_last_error().decode()
        self.a = np.ctypeslib.as_array((ctype * n).from_address(self.ptr))

    def free(self):
        if self.ptr:
            self.L.dss_host_free(self.ptr)
            self.ptr = None


def _history(batch, F):
    """The same decoder history on any batch: slots 1, 3 and 4 have run 5 frames; 0 and 5 are fresh (silent frames next)."""
    feats = torch.from_numpy(np.stack([synthetic_features(600 + k, F) for k in range(3)])).cuda()
    batch.synthesize_ragged_torch(feats, [5, 5, 5], slots=[1, 3, 4])
    torch.cuda.synchronize()


def _ragged_against_progressive(trace=0):
    from dss_amd import _lib
    from dss_amd.lpcnet import LPCNetBatch, read_progress
    L = _lib.load()
    F = 12
    a, b = LPCNetBatch(6, F), LPCNetBatch(6, F)
    if trace:
        a.enable_trace(trace)
        b.enable_trace(trace)
    _history(a, F)
    _history(b, F)
    slots, counts = [3, 0, 4, 1, 5], [7, 12, 0, 3, 9]          # unsorted; a zero-count row; fresh and continued slots
    feats = torch.from_numpy(np.stack([synthetic_features(700 + k, F) for k in range(5)])).cuda()
    want = a.synthesize_ragged_torch(feats, counts, slots=slots).cpu().numpy()
    pcm, done = _Fine(L, 5 * F * FRAME, C.c_int16), _Fine(L, 5, C.c_int32)
    try:
        pcm.a[:] = 12345                                          # rows beyond their counts stay untouched, as on the device
        b.synthesize_ragged_progress_torch(feats, counts, slots, pcm.ptr, done.ptr)
        torch.cuda.synchronize()
        got = pcm.a.reshape(5, F * FRAME)
        assert list(read_progress(done.ptr, 5)) == counts
        for k, n in enumerate(counts):
            assert np.array_equal(got[k, :n * FRAME], want[k, :n * FRAME]), k
            assert (got[k, n * FRAME:] == 12345).all(), k
        # the state carries on bit-exactly: an ordinary call after the progressive one
        feats2 = torch.from_numpy(np.stack([synthetic_features(800 + k, F) for k in range(5)])).cuda()
        w2 = a.synthesize_ragged_torch(feats2, [F] * 5, slots=[0, 1, 3, 4, 5]).cpu().numpy()
        g2 = b.synthesize_ragged_torch(feats2, [F] * 5, slots=[0, 1, 3, 4, 5]).cpu().numpy()
        assert np.array_equal(w2, g2)
    finally:
        torch.cuda.synchronize()
        pcm.free(); done.free()


def test_progressive_call_is_bit_identical_to_the_ragged_call():
    from dss_amd import lpcnet
    lpcnet.load_model(synthetic_blob(0))
    assert lpcnet.model_info()["fast_path"] == 1
    _ragged_against_progressive()


def test_progressive_call_on_the_extended_and_generic_kernels():
    from dss_amd import lpcnet
    try:
        lpcnet.load_model(synthetic_blob(0, skew=0.1))            # z/r tails, long h lists: the EXT instantiation
        assert lpcnet.model_info()["fast_path"] == 2
        _ragged_against_progressive()
        lpcnet.load_model(synthetic_blob(0))
        _ragged_against_progressive(trace=16)                     # 16: the generic kernel, no trace
    finally:
        lpcnet.load_model(synthetic_blob(0))


def test_counters_advance_while_the_kernel_runs_and_cover_their_pcm():
    """Counters read every ~0.5 ms while the launch runs: they take several values strictly between 0 and the count before the
    stream's event completes, never decrease, and whenever one reads v the first v*160 samples already on the host are the final
    PCM (the kernel's stores are visible before the counter that covers them)."""
    from dss_amd import _lib, lpcnet
    from dss_amd.lpcnet import LPCNetBatch, read_progress
    lpcnet.load_model(synthetic_blob(0))
    L = _lib.load()
    R, F = 3, 320
    counts = [F, 300, F - 7]
    a, b = LPCNetBatch(R, F), LPCNetBatch(R, F)
    feats = torch.from_numpy(np.stack([synthetic_features(900 + k, F) for k in range(R)])).cuda()
    want = a.synthesize_ragged_torch(feats, counts, slots=[0, 1, 2]).cpu().numpy()
    stream, ev = L.dss_stream_create(), L.dss_event_create()
    pcm, done = _Fine(L, R * F * FRAME, C.c_int16), _Fine(L, R, C.c_int32)
    snaps = []
    try:
        b.synthesize_ragged_progress_torch(feats, counts, [0, 1, 2], pcm.ptr, done.ptr, stream=stream)
        _lib.check(L.dss_event_record(ev, stream))
        rows = pcm.a.reshape(R, F * FRAME)
        last = np.zeros(R, dtype=np.int32)
        v = np.empty(R, dtype=np.int32)
        while _lib.check(L.dss_event_query(ev)) == 0:
            read_progress(done.ptr, R, v)
            for k in range(R):
                assert v[k] >= last[k], (k, v[k], last[k])
                if v[k] != last[k]:
                    snaps.append((k, int(v[k]), rows[k, : v[k] * FRAME].copy()))
            last[:] = v
            time.sleep(0.0005)
        assert list(read_progress(done.ptr, R)) == counts
        for k, n in enumerate(counts):
            assert np.array_equal(rows[k, : n * FRAME], want[k, : n * FRAME]), k
        for k, n in enumerate(counts):
            inner = {val for kk, val, _ in snaps if kk == k and 0 < val < n}
            assert len(inner) >= 3, (k, sorted(inner))
        for k, val, got in snaps:
            assert np.array_equal(got, want[k, : val * FRAME]), (k, val)
    finally:
        L.dss_stream_synchronize(stream)
        pcm.free(); done.free()
        L.dss_event_destroy(ev)
        L.dss_stream_destroy(stream)


def test_progressive_call_refuses_unsuitable_buffers_and_modes():
    """Pageable memory, cached page-locked memory, a short block, trace, teacher forcing and null pointers: DSS_EINVAL with a
    message, and nothing enqueued (counters and PCM untouched, the decoder state what an identical batch has)."""
    from dss_amd import _lib, lpcnet
    from dss_amd.lpcnet import LPCNetBatch
    lpcnet.load_model(synthetic_blob(0))
    L = _lib.load()
    F = 4
    a, b = LPCNetBatch(2, F), LPCNetBatch(2, F)
    feats = torch.from_numpy(np.stack([synthetic_features(950 + k, F) for k in range(2)])).cuda()
    counts = np.array([F, F], dtype=np.int32)
    pcm, done = _Fine(L, 2 * F * FRAME, C.c_int16), _Fine(L, 2, C.c_int32)
    cached = L.dss_host_alloc(2 * F * FRAME * 2, 1)
    pageable_pcm = np.zeros(2 * F * FRAME, dtype=np.int16)
    pageable_done = np.zeros(2, dtype=np.int32)
    short = _Fine(L, F * FRAME, C.c_int16)                       # one row's worth for a two-row call

    def call(batch, p, d):
        return L.dss_lpcnet_batch_synthesize_ragged_progress_dev(batch._h, feats.data_ptr(), None, counts.ctypes.data, 2, F, 20,
                                                                 p, d, None)
    try:
        done.a[:] = 77
        pcm.a[:] = 5
        cases = [(pageable_pcm.ctypes.data, done.ptr, "dss_host_alloc_fine"), (pcm.ptr, pageable_done.ctypes.data, "dss_host_alloc_fine"),
                 (cached, done.ptr, "dss_host_alloc_fine"), (short.ptr, done.ptr, "dss_host_alloc_fine"),
                 (pcm.ptr + 2, done.ptr, "aligned"), (None, done.ptr, "null"), (pcm.ptr, None, "null")]
        for p, d, msg in cases:
            assert call(b, p, d) == DSS_EINVAL, msg
            assert msg in L.dss_last_error().decode(), L.dss_last_error().decode()
        b.enable_trace(1)
        assert call(b, pcm.ptr, done.ptr) == DSS_EINVAL and "trace" in L.dss_last_error().decode()
        b.force_excitation(np.zeros((2, F * FRAME), dtype=np.uint8), F)
        assert call(b, pcm.ptr, done.ptr) == DSS_EINVAL and "teacher forcing" in L.dss_last_error().decode()
        b.force_excitation(None, F)
        b.enable_trace(0)
        torch.cuda.synchronize()
        assert (done.a == 77).all() and (pcm.a == 5).all()
        # nothing ran on b: its state is still an untouched batch's
        want = a.synthesize_ragged_torch(feats, counts, slots=[0, 1]).cpu().numpy()
        assert call(b, pcm.ptr, done.ptr) == 0
        torch.cuda.synchronize()
        assert np.array_equal(pcm.a.reshape(2, -1), want) and list(done.a) == [F, F]
    finally:
        torch.cuda.synchronize()
        pcm.free(); done.free(); short.free()
        L.dss_host_free(cached)


def _check_chunks(chunks, want, whole):
    """chunks from poll_chunks against the blocking path's segments `want` [(stream, previous_frames, pcm)] and poll()'s `whole`."""
    by = {}
    for s, p, pcm in want:
        by.setdefault(s, []).append((p, pcm))
    pieces, order = {}, {}
    multi = 0
    for s, tag, off, pcm, last in chunks:
        assert pcm.dtype == np.int16
        seq = order.setdefault(s, [])
        if not seq or seq[-1][1]:                                 # the previous segment of this stream is complete
            seq.append([tag, False])
        assert seq[-1][0] == tag, (s, tag, seq[-1])               # no piece of a stream's next segment before the last of this one
        got = pieces.setdefault((s, len(seq) - 1), [])
        assert off == sum(len(x) for x in got), (s, tag, off)     # contiguous from 0
        got.append(pcm)
        seq[-1][1] = last
    for s, segs in by.items():
        assert [t for t, _ in order.get(s, [])] == [p for p, _ in segs], s      # per stream: closing order, each exactly once
        assert all(done for _, done in order[s])
        for k, (_, pcm) in enumerate(segs):
            parts = pieces[(s, k)]
            multi += len(parts) >= 2
            assert np.array_equal(np.concatenate(parts), pcm), (s, k)
    assert set(order) <= set(by)
    # poll()'s whole segments are what they are without the option
    wb = {}
    for s, p, pcm in whole:
        wb.setdefault(s, []).append((p, pcm))
    assert {s: [p for p, _ in v] for s, v in wb.items()} == {s: [p for p, _ in v] for s, v in by.items()}
    for s in by:
        assert all(np.array_equal(x, y) for (_, x), (_, y) in zip(wb[s], by[s]))
    return multi


def test_progressive_queue_pieces_concatenate_to_the_blocking_path():
    """The set-up of test_gpu_gate's asynchronous-against-blocking test (12 streams; lanes / rows per job 3/32, 1/2 and 2/1 with a
    pool of three buffers) with progressive=True: per segment the pieces concatenate to the blocking path's PCM, offsets run
    contiguously from 0, one last piece each, a stream's pieces in order; poll() is unchanged; some segment came in pieces."""
    from dss_amd import lpcnet
    from dss_amd.pipeline import GatedStreamingPipeline
    from test_gpu_gate import _ThresholdVAD, _loud_quiet
    lpcnet.load_model(synthetic_blob(0))
    S, C_, ticks = 12, 64, 90
    rng = np.random.default_rng(77)
    env = _loud_quiet(rng, S, ticks * 40, 20.0, 400.0, 120, 420)
    ecog = rng.standard_normal((S, ticks * 40, C_)) * env[:, :, None]
    kw = dict(buffer_size=300, context_frames=8, channel_means=np.full(C_, 7.4), vad=_ThresholdVAD(), max_segment_frames=300)
    ref = GatedStreamingPipeline(S, C_, asynchronous=False, **kw)
    want = []
    for k in range(ticks):
        want += ref.push(ecog[:, k * 40:(k + 1) * 40])
    assert len(want) >= 20
    ref.close()
    multi = 0
    for lanes, rows, pool in ((3, 32, None), (1, 2, None), (2, 1, 3)):
        pipe = GatedStreamingPipeline(S, C_, asynchronous=True, n_lanes=lanes, rows_per_job=rows, pool_rows=pool, progressive=True, **kw)
        whole, chunks = [], []
        for k in range(ticks):
            whole += pipe.push(ecog[:, k * 40:(k + 1) * 40])
            chunks += pipe.poll_chunks()
            time.sleep(0.002)                                     # let jobs run between ticks, as a paced host does
            chunks += pipe.poll_chunks()
        whole += pipe.flush()
        chunks += pipe.poll_chunks()
        assert pipe.queue.in_flight == 0 and len(whole) == len(want)
        multi += _check_chunks(chunks, want, whole)
        q = pipe.queue
        assert len(q.first_pcm_latencies_ms) == len(q.launch_to_first_pcm_ms) == len(q.lane_wait_ms) == len(want)
        pipe.close()
    assert multi >= 1


def test_progressive_queue_at_128_streams():
    """BASELINE config 5 sizes (128 streams, the reference's detector and decoder architectures, default lanes) with
    progressive=True: every segment's pieces concatenate to the blocking path's PCM, in order, one last piece each."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gated_leg
    from dss_amd import lpcnet
    from dss_amd.pipeline import GatedStreamingPipeline
    lpcnet.load_model(synthetic_blob(0))
    S, ticks = 128, 110
    packets = gated_leg.make_input()[:ticks]
    kw = dict(channel_means=np.full(64, 5.0), max_segment_frames=600)
    ref = GatedStreamingPipeline(S, 64, vad=gated_leg.detector(), asynchronous=False, **kw)
    pipe = GatedStreamingPipeline(S, 64, vad=gated_leg.detector(), progressive=True, **kw)
    want, whole, chunks = [], [], []
    for k in range(ticks):
        want += ref.push(packets[k])
        whole += pipe.push(packets[k])
        chunks += pipe.poll_chunks()
    whole += pipe.flush()
    chunks += pipe.poll_chunks()
    assert len(want) >= 20 and len(whole) == len(want)
    assert _check_chunks(chunks, want, whole) >= 1
    ref.close(); pipe.close()
