"""The scalar side of the one-utterance sample kernel (csrc/lpcnet_sample.hip) around barrier B.  Wave 6 owns the kiss99 generator:
it draws the sample's eight thresholds once it has handed segment 3 of the GRU B relay over (L.thr, read behind barrier C of the
same sample) and saves the generator's state at the end of the call; wave 7 forms GRU B's recurrent half between barriers D and
B, pinned there, and keeps the history shift, de-emphasis and PCM bookkeeping.  These tests cross every seam of that at the
smallest shapes that have one: the frame boundary and the call's last sample (4 frames = 2 silent + 2 synthesised), calls that
start on the first-sample path with the generator, de-emphasis memory, history and GRU B state the call before saved, ragged
rows and a slot reset, the extended, traced / teacher-forced and progressive instantiations -- and one call of the pair kernel,
which shares the header.  Everything is array_equal against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from dss_amd.lpcnet_weights import synthetic_blob, synthetic_features
from test_gpu_lpcnet import _oracle_pcm, model  # noqa: F401  (the module-scoped model fixture of the LPCNet parity tests)

pytestmark = pytest.mark.gpu

ROWS, F_MAX, FRAME = 3, 5, 160


@pytest.fixture(scope="module")
def feats():
    return np.stack([synthetic_features(1500 + b, F_MAX) for b in range(ROWS)])


@pytest.fixture(scope="module")
def ref(oracle, model, feats):     # noqa: F811
    """Per row: the oracle's excitation indices and pre-quantised samples of the three synthesised frames, and its PCM of all
    five (one fresh decoder per row, computed once; the decoder is causal, so k frames of a row are the first k * 160 values)."""
    n = (F_MAX - 2) * FRAME
    out = []
    for b in range(ROWS):
        dec = oracle.decoder(model, trace_cap=F_MAX * FRAME)
        pcm = np.concatenate([dec.synthesize(feats[b, t]) for t in range(F_MAX)])
        out.append((np.array(dec.trace_exc[:n]), np.array(dec.trace_pcm[:n]), pcm))
    return out


def test_one_call_crosses_a_frame_boundary_and_the_last_sample(model, feats, ref):     # noqa: F811
    """2 utterances x 4 frames: sample 159 of the first synthesised frame must be in that frame's copy-out, the LPC switch
    between the frames, and the last sample of the call (no next sample to speculate for).  Timed and traced instantiations;
    the traced one also gives the index and the pre-quantised value of every sample."""
    from dss_amd.lpcnet import LPCNetBatch
    pcm = LPCNetBatch(2, 4).synthesize(feats[:2, :4])
    for b in range(2):
        assert np.array_equal(pcm[b], ref[b][2][:4 * FRAME]), b
    gpu = LPCNetBatch(2, 4)
    gpu.enable_trace(True)
    pcm = gpu.synthesize(feats[:2, :4])
    for b in range(2):
        assert np.array_equal(gpu.tap(b, 3, 4).reshape(-1)[320:].astype(np.uint8), ref[b][0][:320]), b
        assert np.array_equal(gpu.tap(b, 4, 4).reshape(-1)[320:], ref[b][1][:320]), b
        assert np.array_equal(pcm[b], ref[b][2][:4 * FRAME]), b


@pytest.mark.parametrize("split", [(1, 1, 1, 1), (3, 1)])
def test_split_calls_continue_exactly(model, feats, ref, split):     # noqa: F811
    """The same 4 frames as four one-frame calls and as 3 + 1: every call with a synthesised frame starts on the first-sample
    path, from the generator state (saved by wave 6), de-emphasis memory, history and GRU B state the call before saved."""
    from dss_amd.lpcnet import LPCNetBatch
    gpu = LPCNetBatch(2, max(split))
    one = LPCNetBatch(2, 4).synthesize(feats[:2, :4])
    parts, t = [], 0
    for n in split:
        parts.append(gpu.synthesize(feats[:2, t:t + n]))
        t += n
    got = np.concatenate(parts, axis=1)
    for b in range(2):
        assert np.array_equal(got[b], one[b]), (split, b)
        assert np.array_equal(got[b], ref[b][2][:4 * FRAME]), (split, b)


def test_ragged_rows_and_a_single_slot_reset(model, feats, ref):     # noqa: F811
    """Rows of 3, 4 and 5 frames on slots that are not their row numbers (the RAGGED instantiation: each workgroup ends at its
    own frame); then slot 0 alone is reset and a second call runs a fresh utterance on it beside a continued one."""
    from dss_amd.lpcnet import LPCNetBatch
    counts, slots = [3, 4, 5], [2, 0, 1]
    gpu = LPCNetBatch(3, F_MAX)
    got = gpu.synthesize_ragged([feats[b, :counts[b]] for b in range(3)], slots=slots)
    for b in range(3):
        assert np.array_equal(got[b], ref[b][2][:counts[b] * FRAME]), b
    gpu.reset(0)                                                   # held row 1; slot 2 (row 0, three frames so far) carries on
    got = gpu.synthesize_ragged([feats[1, :3], feats[0, 3:5]], slots=[0, 2])
    assert np.array_equal(got[0], ref[1][2][:3 * FRAME])
    assert np.array_equal(got[1], ref[0][2][3 * FRAME:5 * FRAME])


def test_extended_path_model_at_four_frames(oracle):
    """The EXT instantiation, built as test_gpu_lpcnet_walk.py::test_extended_path_model builds it."""
    from dss_amd import lpcnet
    from dss_amd.lpcnet import LPCNetBatch
    blob = synthetic_blob(0, skew=0.1)
    try:
        lpcnet.load_model(blob)
        assert lpcnet.model_info()["fast_path"] == 2
        f = np.stack([synthetic_features(840 + b, 4) for b in range(2)])
        assert np.array_equal(LPCNetBatch(2, 4).synthesize(f), _oracle_pcm(oracle, blob, f))
    finally:
        lpcnet.load_model(synthetic_blob(0))


def test_teacher_forced_logits_pin_the_thresholds_and_the_recurrent_half(oracle, model, feats):     # noqa: F811
    """3 frames, one of them synthesised: with the excitation forced on both sides all 255 logits of every sample equal the
    oracle's (they are GRU B's output, so a recurrent half formed from the wrong state shows at once), and so do the
    pre-quantised samples and the PCM."""
    from dss_amd.lpcnet import LPCNetBatch
    B, F = 2, 3
    n = F * FRAME
    exc = np.clip(np.rint(128 + np.random.default_rng(23).normal(0, 30, (B, n))), 0, 255).astype(np.uint8)
    gpu = LPCNetBatch(B, F)
    gpu.enable_trace(1)
    gpu.force_excitation(exc, F)
    pcm = gpu.synthesize(feats[:B, :F])
    for b in range(B):
        dec = oracle.decoder(model, trace_cap=n)
        dec.force(exc[b, 320:])
        want = np.concatenate([dec.synthesize(feats[b, t]) for t in range(F)])
        logits = gpu.tap(b, 5, F).reshape(n, 256)[320:]
        assert np.array_equal(logits, dec.forced_logits), (b, np.abs(logits - dec.forced_logits).max())
        assert np.array_equal(gpu.tap(b, 4, F).reshape(-1)[320:], dec.trace_pcm[:n - 320]), b
        assert np.array_equal(pcm[b], want), b


def test_progressive_chunks_concatenate_to_the_whole_call(model, feats, ref):     # noqa: F811
    """The PROGRESS instantiation, 2 rows x 4 frames: the pieces the frame counters announce, taken from the host block,
    concatenate to the PCM of the whole call (and the oracle's)."""
    import torch
    from dss_amd import _lib
    from dss_amd.lpcnet import LPCNetBatch, read_progress
    from dss_amd.segment_queue import progress_chunks
    L = _lib.load()
    R, F = 2, 4
    whole = LPCNetBatch(R, F).synthesize(feats[:R, :F])
    ptr_pcm, ptr_done = L.dss_host_alloc_fine(R * F * FRAME * 2), L.dss_host_alloc_fine(R * 4)
    assert ptr_pcm and ptr_done, L.dss_last_error().decode()
    try:
        host = np.ctypeslib.as_array((C.c_int16 * (R * F * FRAME)).from_address(ptr_pcm)).reshape(R, F * FRAME)
        host[:] = 12345
        np.ctypeslib.as_array((C.c_int32 * R).from_address(ptr_done))[:] = 0
        dev = torch.from_numpy(np.ascontiguousarray(feats[:R, :F])).cuda()
        LPCNetBatch(R, F).synthesize_ragged_progress_torch(dev, [F] * R, [0, 1], ptr_pcm, ptr_done)
        torch.cuda.synchronize()
        counters = read_progress(ptr_done, R)
        assert list(counters) == [F] * R
        sent, pieces = [0] * R, [[] for _ in range(R)]
        for c in range(1, F + 1):                                  # the counters as a reader sees them pass: a frame at a time
            for k, f0, f1, last in progress_chunks([F] * R, sent, np.minimum(counters, c)):
                pieces[k].append(host[k, f0 * FRAME:f1 * FRAME].copy())
                assert last == (c == F)
        assert all(len(p) == F for p in pieces)
        for k in range(R):
            got = np.concatenate(pieces[k])
            assert np.array_equal(got, whole[k]) and np.array_equal(got, ref[k][2][:F * FRAME]), k
    finally:
        torch.cuda.synchronize()
        L.dss_host_free(ptr_pcm)
        L.dss_host_free(ptr_done)


def test_pair_kernel_one_row_three_frames(model, feats, ref):     # noqa: F811
    """The pair kernel shares lpcnet_sample_common.h with the kernel above: one row (the smallest call it takes, the second
    half of its workgroup idle) x 3 frames still equals the oracle."""
    from dss_amd.lpcnet import LPCNetBatch
    gpu = LPCNetBatch(1, 3)
    gpu.set_multi(2)
    assert np.array_equal(gpu.synthesize(feats[:1, :3])[0], ref[0][2][:3 * FRAME])
