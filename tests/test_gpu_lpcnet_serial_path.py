"""GPU parity, tolerance 0, of what the sample kernels run between barriers D and B once the slots their results do not need
are gone (csrc/lpcnet_sample.hip, DSS_SERIAL_SLOTS): the heap-form tree walk, role A compiled for its wave's z/r list length
(the role's capacity, one pair of slots below it, or any length), scalar row offsets of the embedding loads, hand-over tags
written ahead of a segment's last sums.  The order of the GRU A sums stays the model's run-time flag; both orders run here.

  walk        every excitation value forced through the tree (all 256, then 64 seeded ones) on two rows: the kernels' own walk
              must return the forced value (excitation trace) and everything downstream of it the oracle's PCM.  One-utterance,
              pair and generic kernel.  tests/test_cpu_tree_walk.py proves the two instruction sequences equal on the CPU.
  order x     every case of tests/lpcnet_layouts.py that changes z/r block counts, and one more whose lightest wave has no z/r
  lengths     block at all, each packed with gru_a_order 0 and 1: free-running, a uniform and a ragged call.  The lengths a wave
              runs: 0 ('zr_wave_empty'), 2 .. 12 ('reversed'), 6 on every wave (the base counts), 8 on waves 0..3 at capacity
              ('w03_8'), 10 and 12 on waves 4, 5 ('z10', 'z11', 'z12_r', 'z12x16'), tails on the extended paths ('z13', 'w03_9',
              'tail16_w45', 'tail16_w03') and the generic kernel's lists ('tail17_w45', 'tail17_w03').  On these inputs the oracle's
              PCM is the same for both orders (they differ in the last bits of the logits, which rarely move a sample): what the
              PCM proves per order is that the kernel chosen for it runs the lists right; that the order itself is the model's
              is proved on the logits by test_gpu_lpcnet.py::test_gru_a_recurrent_first_order_flag and the *_order1 cases of
              test_gpu_lpcnet_layouts.py.
  hand-over   one row, three frames, called twice on the carried state: the sample number in the relay's tags starts again in the
              second call.
"""
import warnings

import numpy as np
import pytest

import lpcnet_layouts as Y
from dss_amd.lpcnet_weights import GRUA_INPUT_FIRST, GRUA_RECUR_FIRST, make_synthetic_weights, pack_blob, synthetic_blob, synthetic_features

pytestmark = pytest.mark.gpu

ROWS, FRAMES = 2, 4                        # two silent frames plus 320 samples
ZR_CASES = ["z10", "z11", "z12_r", "z12x16", "z13", "w03_8", "w03_9", "tail16_w45", "tail17_w45", "tail16_w03", "tail17_w03",
            "reversed", "ties", "zr_wave_empty"]
EMPTY_GROUPS = (3, 9, 14, 20, 27, 33, 40, 46)          # eight row groups without z and r blocks: the lightest, so wave 0's


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.nonzero(~(got.reshape(-1) == want.reshape(-1)))[0]
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at {k}: kernel {got.reshape(-1)[k]!r} "
                             f"oracle {want.reshape(-1)[k]!r}")


def _weights(name):
    if name == "zr_wave_empty":
        counts = [0 if g in EMPTY_GROUPS else 5 for g in range(48)]
        return Y.shaped(make_synthetic_weights(0), counts, counts, None)
    return Y.build(name)[0]


def _fits(name):
    """(fast_path, pair_fits) of a case; the extra case is a plain 10-slot model well inside the pair kernel's limit."""
    return (1, True) if name == "zr_wave_empty" else (Y.CASES[name].fast_path, Y.CASES[name].pair_fits)


def _features():
    return Y.features(ROWS, FRAMES)


def _batch(rows, frames):
    from dss_amd.lpcnet import LPCNetBatch
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # the models beyond the outer capacities announce the generic kernel
        return LPCNetBatch(rows, frames)


def _restore():
    from dss_amd import lpcnet
    lpcnet.load_model(synthetic_blob(0))


# ---- walk ---------------------------------------------------------------------------------------------------------------
def _walk_excitation():
    """(ROWS, FRAMES * 160) uint8: behind the two silent frames all 256 values -- ascending on row 0, a seeded permutation on
    row 1 -- then 64 seeded ones."""
    rng = np.random.default_rng(4242)
    exc = np.zeros((ROWS, FRAMES * 160), np.uint8)
    exc[0, 320:576] = np.arange(256)
    exc[1, 320:576] = rng.permutation(256)
    exc[:, 576:] = rng.integers(0, 256, (ROWS, 64))
    return exc


_walk_ref = []


def _walk_reference(oracle):
    if not _walk_ref:
        m = oracle.lpcnet_model(synthetic_blob(0))
        feats, exc = _features(), _walk_excitation()
        pcm = []
        for b in range(ROWS):
            dec = oracle.decoder(m, trace_cap=FRAMES * 160)
            dec.force(exc[b, 320:])
            pcm.append(np.concatenate([dec.synthesize(feats[b, t]) for t in range(FRAMES)]))
        _walk_ref.append((feats, exc, pcm))
    return _walk_ref[0]


@pytest.mark.parametrize("kernel", ["one", "pair", "generic"])
def test_walk_returns_every_forced_value(oracle, kernel):
    _restore()
    feats, exc, want = _walk_reference(oracle)
    gpu = _batch(ROWS, FRAMES)
    gpu.set_multi(2 if kernel == "pair" else -1)
    gpu.enable_trace(17 if kernel == "generic" else 1)
    gpu.force_excitation(exc, FRAMES)
    pcm = gpu.synthesize(feats)
    for b in range(ROWS):
        _same(gpu.tap(b, 3, FRAMES).reshape(-1)[320:].astype(np.uint8), exc[b, 320:], f"{kernel} kernel / row {b} / excitation")
        _same(pcm[b], want[b], f"{kernel} kernel / row {b} / PCM")


# ---- order x list lengths -------------------------------------------------------------------------------------------------
_zr_ref = {}


def _zr_reference(oracle, name, order):
    """(blob, features, free-running oracle PCM per row), computed once per model."""
    if (name, order) not in _zr_ref:
        blob = pack_blob(_weights(name), gru_a_order=order)
        m = oracle.lpcnet_model(blob)
        feats = _features()
        pcm = []
        for b in range(ROWS):
            dec = oracle.decoder(m)
            pcm.append(np.concatenate([dec.synthesize(feats[b, t]) for t in range(FRAMES)]))
        _zr_ref[(name, order)] = (blob, feats, pcm)
    return _zr_ref[(name, order)]


def _kernels(name):
    fast, pair = _fits(name)
    ks = [("auto", -1, False), ("generic", -1, True)]
    if pair:
        ks.append(("pair", 2, False))
    return ks


@pytest.mark.parametrize("order", [GRUA_INPUT_FIRST, GRUA_RECUR_FIRST])
@pytest.mark.parametrize("name", ZR_CASES)
def test_order_and_list_lengths_uniform(oracle, name, order):
    from dss_amd import lpcnet
    try:
        blob, feats, want = _zr_reference(oracle, name, order)
        lpcnet.load_model(blob)
        info = lpcnet.model_info()
        assert info["fast_path"] == _fits(name)[0] and info["gru_a_order"] == order, (name, order, info)
        for label, multi, generic in _kernels(name):
            gpu = _batch(ROWS, FRAMES)
            gpu.set_multi(multi)
            if generic:
                gpu.enable_trace(16)
            pcm = gpu.synthesize(feats)
            for b in range(ROWS):
                _same(pcm[b], want[b], f"{name} / order {order} / {label} kernel / row {b} / PCM")
    finally:
        _restore()


@pytest.mark.parametrize("order", [GRUA_INPUT_FIRST, GRUA_RECUR_FIRST])
@pytest.mark.parametrize("name", ZR_CASES)
def test_order_and_list_lengths_ragged(oracle, name, order):
    """Rows of 4 and 3 frames whose slot list swaps them, then the shorter slot's last frame on the carried state."""
    from dss_amd import lpcnet
    calls = [[(1, 0, 4), (0, 0, 3)], [(0, 3, 1)]]               # (slot, first frame, frames), rows in this order
    try:
        blob, feats, want = _zr_reference(oracle, name, order)
        lpcnet.load_model(blob)
        for label, multi, generic in _kernels(name):
            if generic:
                continue
            gpu = _batch(ROWS, FRAMES)
            gpu.set_multi(multi)
            for c, rows in enumerate(calls):
                got = gpu.synthesize_ragged([feats[s, a:a + k] for s, a, k in rows], slots=[s for s, _, _ in rows], longest_first=False)
                for (s, a, k), pcm in zip(rows, got):
                    _same(pcm, want[s][a * 160:(a + k) * 160], f"{name} / order {order} / {label} kernel / ragged call {c} / slot {s}")
    finally:
        _restore()


# ---- hand-over --------------------------------------------------------------------------------------------------------------
def test_relay_tags_restart_on_carried_state(oracle):
    _restore()
    F = 3
    feats = np.stack([synthetic_features(6200, 2 * F)])
    m = oracle.lpcnet_model(synthetic_blob(0))
    dec = oracle.decoder(m)
    want = np.concatenate([dec.synthesize(feats[0, t]) for t in range(2 * F)])
    gpu = _batch(1, F)
    gpu.set_multi(-1)
    first = gpu.synthesize(feats[:, :F])
    second = gpu.synthesize(feats[:, F:])
    _same(first[0], want[:F * 160], "first call / PCM")
    _same(second[0], want[F * 160:], "second call on the carried state / PCM")
