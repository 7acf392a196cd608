"""GPU parity of the LPCNet kernels against the (unflushed) CPU oracle on models OUTSIDE the well-conditioned regime of
make_synthetic_weights: saturated gates ('hot'), decided sampling at the ends of the tree and of the int16 range ('peaked'),
subnormal weights / states / products ('tiny'), row groups of GRU A without blocks ('empty', 'empty_gate', 'empty_skewed').
Models and inputs come from tests/lpcnet_regimes.py; tests/test_cpu_lpcnet_regimes.py proves on the oracle alone that every
input used here reaches its regime and stays finite (Inf / NaN are outside the parity contract: `(int)floor(NaN)` is
undefined in the C source).  Everything is compared with array_equal, tolerance 0, like the rest of the LPCNet suite.

Kernel per case (lpcnet_regimes.CASES, asserted from model_info()): fast_path 1, the CU-resident kernel, for all but
'empty_skewed', which needs the extended paths (fast_path 2) and is therefore refused by the pair kernel ("do not fit").
The blob loader accepts every variant, a gate without a single block included ('empty_gate'): it is a legal model."""
import numpy as np
import pytest

import lpcnet_regimes as R
from dss_amd.lpcnet_weights import GRUA_RECUR_FIRST, synthetic_blob

pytestmark = pytest.mark.gpu

_ref = {}


def _blob(oracle, name, order=0):
    table = oracle.lpcnet_table(oracle.lpcnet_model(synthetic_blob(0)), 1, 256)
    return R.build(name, table, gru_a_order=order)[1]


def _reference(oracle, name, order=0):
    """Oracle results of a case (cached): per row the PCM, the sampled excitation and the pre-quantised value."""
    key = (name, order)
    if key not in _ref:
        blob = _blob(oracle, name, order)
        m = oracle.lpcnet_model(blob)
        feats = R.features(name)
        B, F = feats.shape[:2]
        rows = []
        for b in range(B):
            dec = oracle.decoder(m, trace_cap=F * 160)
            pcm = np.concatenate([dec.synthesize(feats[b, t]) for t in range(F)])
            rows.append((pcm, dec.trace_exc[:(F - 2) * 160].copy(), dec.trace_pcm[:(F - 2) * 160].copy()))
        _ref[key] = (blob, m, feats, rows)
    return _ref[key]


def _same(got, want, what):
    """array_equal with a message that names the first differing element and both values."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.nonzero(~(got.reshape(-1) == want.reshape(-1)))[0]          # a NaN on either side counts as a difference
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at {k}: kernel {got.reshape(-1)[k]!r} "
                             f"oracle {want.reshape(-1)[k]!r}")
    return got.size


def _kernels(name):
    """(label, set_multi, generic): the automatic choice, the generic kernel forced, the pair kernel where the model fits."""
    ks = [("auto", 0, False), ("generic", 0, True)]
    if R.CASES[name] == 1:
        ks.append(("pair", 2, False))
    return ks


def _load(oracle, name, order=0):
    from dss_amd import lpcnet
    blob = _reference(oracle, name, order)[0]
    lpcnet.load_model(blob)
    info = lpcnet.model_info()
    assert info["fast_path"] == R.CASES[name], (name, info)
    assert info["gru_a_order"] == order
    return info


def _restore():
    from dss_amd import lpcnet
    lpcnet.load_model(synthetic_blob(0))


@pytest.mark.parametrize("name", list(R.CASES))
def test_free_running_every_kernel(oracle, name):
    """Sampled excitation, pre-quantised value and int16 PCM of every row, on the automatic, the generic and the pair
    kernel, each in its plain and in its traced instantiation; the pair kernel with an odd (5) and an even (4) number of
    rows, every row with its own features and cepstral gain (the two halves of a packed instruction differ in magnitude)."""
    from dss_amd import _lib
    from dss_amd.lpcnet import LPCNetBatch
    try:
        _load(oracle, name)
        _, _, feats, rows = _reference(oracle, name)
        B, F = feats.shape[:2]
        compared = 0
        for label, multi, generic in _kernels(name):
            for nrows in ((B, B - 1) if multi == 2 else (B,)):
                for trace in (False, True):
                    gpu = LPCNetBatch(nrows, F)
                    if multi:
                        gpu.set_multi(multi)
                    if generic:
                        gpu.enable_trace(17 if trace else 16)
                    elif trace:
                        gpu.enable_trace(1)
                    pcm = gpu.synthesize(feats[:nrows])
                    for b in range(nrows):
                        tag = f"{name} / {label} kernel{' traced' if trace else ''} / {nrows} rows / row {b}"
                        if trace:
                            _same(gpu.tap(b, 3, F).reshape(-1)[320:].astype(np.uint8), rows[b][1], tag + " / excitation")
                            _same(gpu.tap(b, 4, F).reshape(-1)[320:], rows[b][2], tag + " / pre-quantised value")
                        compared += _same(pcm[b], rows[b][0], tag + " / PCM")
        if R.CASES[name] != 1:
            gpu = LPCNetBatch(B, F)
            with pytest.raises(_lib.DssError, match="do not fit"):
                gpu.set_multi(2)
        print(f"{name}: {compared} PCM samples compared, all equal")
    finally:
        _restore()


@pytest.mark.parametrize("name", list(R.CASES))
def test_ragged_rows_zero_length_row_and_carried_state(oracle, name):
    """Two ragged calls on one batch object: the first has a zero-length row, the second continues every slot (its first
    frames are not silent) next to a fresh one; on the automatic and on the pair kernel (rows in the caller's order, so
    the pairs are the ones written here).  One oracle decoder per slot is the reference."""
    from dss_amd.lpcnet import LPCNetBatch
    calls = [[(0, 0, 5), (1, 0, 0), (2, 0, 3), (3, 0, 4)],                  # (slot, first frame, frames)
             [(0, 5, 3), (1, 0, 4), (2, 3, 5), (3, 4, 2), (4, 0, 8)]]
    try:
        _load(oracle, name)
        _, m, feats, _ = _reference(oracle, name)
        B, F = feats.shape[:2]
        for label, multi, generic in _kernels(name):
            if generic:
                continue
            gpu = LPCNetBatch(B, F)
            if multi:
                gpu.set_multi(multi)
            decs = [oracle.decoder(m) for _ in range(B)]
            for c, rows in enumerate(calls):
                got = gpu.synthesize_ragged([feats[s, a:a + n] for s, a, n in rows], slots=[s for s, _, _ in rows],
                                            longest_first=False)
                for (s, a, n), pcm in zip(rows, got):
                    want = [decs[s].synthesize(feats[s, t]) for t in range(a, a + n)]
                    want = np.concatenate(want) if want else np.empty(0, np.int16)
                    _same(pcm, want, f"{name} / {label} kernel / ragged call {c} / slot {s} frames {a}..{a + n}")
    finally:
        _restore()


@pytest.mark.parametrize("name", list(R.CASES))
def test_teacher_forced_logits(oracle, name):
    """Teacher forcing with an excitation that holds long runs of 0 and of 255, swaps between them and noise: all 255 node
    logits of every sample, the excitation index and the pre-quantised value."""
    from dss_amd.lpcnet import LPCNetBatch
    try:
        _load(oracle, name)
        _, m, feats, _ = _reference(oracle, name)
        B, F = 3, feats.shape[1]
        n = F * 160
        exc = R.forced_excitation(B, F)
        want = []
        for b in range(B):
            dec = oracle.decoder(m, trace_cap=n)
            dec.force(exc[b, 320:])
            pcm = np.concatenate([dec.synthesize(feats[b, t]) for t in range(F)])
            assert np.isfinite(dec.forced_logits).all()
            want.append((pcm, dec.forced_logits.copy(), dec.trace_pcm[:n - 320].copy()))
        compared = 0
        for label, multi, generic in _kernels(name):
            gpu = LPCNetBatch(B, F)
            if multi:
                gpu.set_multi(multi)
            gpu.enable_trace(17 if generic else 1)
            gpu.force_excitation(exc, F)
            pcm = gpu.synthesize(feats[:B])
            for b in range(B):
                tag = f"{name} / {label} kernel / teacher forced / row {b}"
                _same(gpu.tap(b, 3, F).reshape(-1)[320:].astype(np.uint8), exc[b, 320:], tag + " / excitation")
                compared += _same(gpu.tap(b, 5, F).reshape(n, 256)[320:], want[b][1], tag + " / node logits (sample*256+node)")
                _same(gpu.tap(b, 4, F).reshape(-1)[320:], want[b][2], tag + " / pre-quantised value")
                _same(pcm[b], want[b][0], tag + " / PCM")
        print(f"{name}: {compared} forced logits compared, all equal")
    finally:
        _restore()


@pytest.mark.parametrize("name", ["hot", "tiny"])
def test_frame_network_taps(oracle, name):
    """The conditioning vectors go through the same table helper ('tiny' makes GRU A's conditioning layer subnormal)."""
    from dss_amd.lpcnet import LPCNetBatch
    try:
        _load(oracle, name)
        _, m, feats, _ = _reference(oracle, name)
        B, F = feats.shape[:2]
        gpu = LPCNetBatch(B, F)
        gpu.synthesize(feats)
        for b in range(B):
            dec = oracle.decoder(m)
            for t in range(F):
                dec.frame_network(feats[b, t])
                tag = f"{name} / frame network / row {b} frame {t}"
                _same(gpu.tap(b, 0, F)[t], dec.tap(0, 1152), tag + " / gru_a_condition")
                _same(gpu.tap(b, 1, F)[t], dec.tap(1, 48), tag + " / gru_b_condition")
                _same(gpu.tap(b, 2, F)[t], dec.tap(2, 16), tag + " / lpc")
    finally:
        _restore()


@pytest.mark.parametrize("name", list(R.ORDER1_CASES))
def test_gru_a_recurrent_first_order(oracle, name):
    """gru_a_order = 1 (the z / r sums associate the other way round), every kernel."""
    from dss_amd.lpcnet import LPCNetBatch
    try:
        _load(oracle, name, GRUA_RECUR_FIRST)
        _, _, feats, rows = _reference(oracle, name, GRUA_RECUR_FIRST)
        B, F = feats.shape[:2]
        for label, multi, generic in _kernels(name):
            gpu = LPCNetBatch(B, F)
            if multi:
                gpu.set_multi(multi)
            if generic:
                gpu.enable_trace(16)
            pcm = gpu.synthesize(feats)
            for b in range(B):
                _same(pcm[b], rows[b][0], f"{name} order 1 / {label} kernel / row {b} / PCM")
    finally:
        _restore()
