"""The hop from the decision bits to the embedding loads of the one-utterance sample kernel: every GRU A wave walks the sampling
tree itself and takes the two speculated mu-law indices of the next sample from SampleLds::spec_tab_idx[exc], a table that
three other groups of waves fill between barriers B and C.  These tests drive every entry of that table (all 256 values, so
every 8-byte group, every 16-bit field in it and both of its words) through the hop, in every instantiation that shares the
text (timed, trace / teacher-forced, ragged, extended) and on the first-sample path that goes round it, against the CPU
oracle at tolerance 0.  They pin the hop for any change of how the entry is fetched or of the order of the three loads."""
import numpy as np
import pytest

from dss_amd.lpcnet_weights import synthetic_blob, synthetic_features
from test_gpu_lpcnet import _oracle_pcm, model  # noqa: F401  (the module-scoped model fixture of the LPCNet parity tests)

pytestmark = pytest.mark.gpu

SEEDS, F_FREE = (0, 1, 2), 8


@pytest.fixture(scope="module")
def free_feats():
    return np.stack([synthetic_features(s, F_FREE) for s in SEEDS])


@pytest.fixture(scope="module")
def free_ref(oracle, model, free_feats):     # noqa: F811
    """The oracle's free-running excitation indices, pre-quantised samples and PCM for the three utterances (computed once)."""
    n = (F_FREE - 2) * 160
    ref = []
    for b in range(len(SEEDS)):
        dec = oracle.decoder(model, trace_cap=F_FREE * 160)
        pcm = np.concatenate([dec.synthesize(free_feats[b, t]) for t in range(F_FREE)])
        ref.append((np.array(dec.trace_exc[:n]), np.array(dec.trace_pcm[:n]), pcm))
    return ref


def test_forced_sweep_takes_every_table_entry_and_field(oracle, model):     # noqa: F811
    """Teacher forcing with exc = k % 256 over 640 synthesised samples per utterance: every one of the 64 groups of four entries,
    the four field positions and both words of a group are taken at least twice.  Forced index, pre-quantised sample, the 255
    logits of every sample (they depend on the two looked-up indices of the sample before) and the PCM: array_equal."""
    from dss_amd.lpcnet import LPCNetBatch
    B, F = 2, 6
    n = F * 160
    feats = np.stack([synthetic_features(300 + b, F) for b in range(B)])
    exc = np.tile((np.arange(n) % 256).astype(np.uint8), (B, 1))
    taken = exc[0, 320:]
    assert np.bincount(taken, minlength=256).min() >= 2 and np.bincount(taken >> 2, minlength=64).min() >= 8
    gpu = LPCNetBatch(B, F)
    gpu.enable_trace(1)
    gpu.force_excitation(exc, F)
    pcm = gpu.synthesize(feats)
    for b in range(B):
        dec = oracle.decoder(model, trace_cap=n)
        dec.force(exc[b, 320:])
        want = np.concatenate([dec.synthesize(feats[b, t]) for t in range(F)])
        assert np.array_equal(dec.trace_exc[:n - 320], exc[b, 320:])
        assert np.array_equal(gpu.tap(b, 3, F).reshape(-1)[320:].astype(np.uint8), exc[b, 320:]), b
        assert np.array_equal(gpu.tap(b, 4, F).reshape(-1)[320:], dec.trace_pcm[:n - 320]), b
        logits = gpu.tap(b, 5, F).reshape(n, 256)[320:]
        assert np.array_equal(logits, dec.forced_logits), (b, np.abs(logits - dec.forced_logits).max())
        assert np.array_equal(pcm[b], want), b


def test_free_running_timed_instantiation(model, free_feats, free_ref):     # noqa: F811
    """Seeds 0, 1, 2 x 8 frames, fresh decoders.  The oracle's own sequence must spread over the table (on the CPU: 126 distinct
    values in 43 distinct groups of four); then the untraced kernel's PCM and the traced kernel's index / sample / PCM equal the oracle's."""
    from dss_amd.lpcnet import LPCNetBatch
    all_exc = np.concatenate([r[0] for r in free_ref]).astype(np.int64)
    assert len(np.unique(all_exc)) >= 96 and len(np.unique(all_exc >> 2)) >= 32, (len(np.unique(all_exc)), len(np.unique(all_exc >> 2)))
    B = len(SEEDS)
    pcm = LPCNetBatch(B, F_FREE).synthesize(free_feats)                  # no trace: the instantiation the benchmark times
    for b in range(B):
        assert np.array_equal(pcm[b], free_ref[b][2]), b
    gpu = LPCNetBatch(B, F_FREE)
    gpu.enable_trace(True)
    pcm = gpu.synthesize(free_feats)
    for b in range(B):
        want_exc, want_pre, want_pcm = free_ref[b]
        assert np.array_equal(gpu.tap(b, 3, F_FREE).reshape(-1)[320:].astype(np.uint8), want_exc), b
        assert np.array_equal(gpu.tap(b, 4, F_FREE).reshape(-1)[320:], want_pre), b
        assert np.array_equal(pcm[b], want_pcm), b


def test_ragged_rows_with_a_slot_list(model, free_feats, free_ref):     # noqa: F811
    """The RAGGED instantiation: three rows of 8 / 5 / 3 frames, each on a decoder slot that is not its row number."""
    from dss_amd.lpcnet import LPCNetBatch
    counts, slots = [8, 5, 3], [2, 0, 1]
    got = LPCNetBatch(3, F_FREE).synthesize_ragged([free_feats[b, :counts[b]] for b in range(3)], slots=slots)
    for b in range(3):
        assert np.array_equal(got[b], free_ref[b][2][:counts[b] * 160]), b


def test_call_split_in_two_takes_the_first_sample_path_twice(model, free_feats, free_ref):     # noqa: F811
    """4 + 4 frames against one call of 8: the second call starts from L.idx behind barrier A, before any table of this call
    exists, and must continue the first call's sequence exactly."""
    from dss_amd.lpcnet import LPCNetBatch
    gpu = LPCNetBatch(len(SEEDS), F_FREE)
    got = np.concatenate([gpu.synthesize(free_feats[:, :4]), gpu.synthesize(free_feats[:, 4:])], axis=1)
    for b in range(len(SEEDS)):
        assert np.array_equal(got[b], free_ref[b][2]), b


def test_extended_path_model(oracle):
    """The EXT instantiation (z/r tail blocks and long h lists from LDS records), built as
    test_extended_paths_ragged_and_teacher_forced builds it: 2 x 6 frames, one uniform call."""
    from dss_amd import lpcnet
    from dss_amd.lpcnet import LPCNetBatch
    blob = synthetic_blob(0, skew=0.1)
    try:
        lpcnet.load_model(blob)
        assert lpcnet.model_info()["fast_path"] == 2
        feats = np.stack([synthetic_features(840 + b, 6) for b in range(2)])
        assert np.array_equal(LPCNetBatch(2, 6).synthesize(feats), _oracle_pcm(oracle, blob, feats))
    finally:
        lpcnet.load_model(synthetic_blob(0))
