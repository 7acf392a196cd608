"""The short table activations of the CU-resident sample kernel (csrc/lpcnet_device.h: dss_sigmoid_short*, dss_tanh_times*).

(a) On the device, through the test-only entry point dss_selftest_tansig: the short forms against the forms they replace
    (dss_tanh_approx / dss_sigmoid_approx, tables in LDS as in the kernel) over ALL 2^32 bit patterns of the argument, single
    and two-at-once forms; and the two-operand fold a * tanh(x) == (sign folded into a) * |tanh(x)| on 2^24 argument
    patterns around each of: zero and the subnormals, the first index boundary, the clamp, large arguments -- each with a
    pseudo-random factor (every exponent, subnormals, +-0).  The entry point returns a mismatch count and the first
    mismatch; the count must be 0 (two NaNs count as equal: a NaN in must give a NaN out).
(b) The kernels that use them against the CPU oracle, array_equal: 3 utterances x 5 frames (two silent, three synthesised)
    through the one-utterance kernel, free running (PCM of the plain instantiation; excitation, pre-quantised value and
    PCM of the traced one) and teacher forced (all 255 node logits of every sample), on
      the seed-0 model; the saturating and the subnormal model of tests/lpcnet_regimes.py; a skewed model, which takes the
      instantiation with the extended paths (that one keeps the plain activations); a model on the 12-slot instantiation;
      the seed-0 model with the RECUR_FIRST order flag.
    The two-utterance kernel keeps the plain activations and is covered by the existing suites."""
import ctypes as C

import numpy as np
import pytest

import lpcnet_regimes as R
from dss_amd.lpcnet_weights import GRUA_RECUR_FIRST, synthetic_blob, synthetic_features

pytestmark = pytest.mark.gpu

ROWS, FRAMES = 3, 5


def _sweep(which, start, n):
    from dss_amd import _lib
    L = _lib.require_gpu()
    res = (C.c_ulonglong * 2)()
    _lib.check(L.dss_selftest_tansig(which, start, n, res))
    count, first = int(res[0]), int(res[1])
    what = ("tanh", "sigmoid", "a * tanh")[which]
    print(f"{what}: {n} patterns from {start:#010x}: {count} mismatches")
    assert count == 0, f"{what}: {count} of {n} patterns differ, first at bits {(start + first) & 0xffffffff:#010x}"
    assert first == 2 ** 64 - 1


@pytest.mark.parametrize("which", [0, 1], ids=["tanh", "sigmoid"])
def test_short_forms_equal_the_table_forms_for_every_fp32_argument(which):
    _sweep(which, 0, 2 ** 32)


@pytest.mark.parametrize("start", [0x00000000, 0x80000000, 0x3ca3d70a - 2 ** 23, 0xbca3d70a - 2 ** 23, 0x41000000 - 2 ** 23,
                                   0xc1000000 - 2 ** 23, 0x4b000000, 0x7f000000],
                         ids=["zero+", "zero-", "first boundary+", "first boundary-", "clamp+", "clamp-", "large", "inf and NaN"])
def test_sign_folded_into_the_factor(start):
    """2^24 consecutive argument patterns from `start`, each with its own pseudo-random finite factor."""
    _sweep(2, start, 2 ** 24)


def test_selftest_rejects_bad_arguments():
    from dss_amd import _lib
    L = _lib.require_gpu()
    res = (C.c_ulonglong * 2)()
    assert L.dss_selftest_tansig(3, 0, 16, res) != 0
    assert L.dss_selftest_tansig(0, 0, 0, res) != 0
    assert L.dss_selftest_tansig(0, 0, 2 ** 32 + 1, res) != 0
    assert L.dss_selftest_tansig(0, 0, 16, None) != 0


# ---- (b) ------------------------------------------------------------------------------------------------------------
def _case(oracle, name):
    """(blob, features (ROWS, FRAMES, 20), fast_path, register slots per gate) of a named model."""
    if name in ("hot", "tiny"):
        table = oracle.lpcnet_table(oracle.lpcnet_model(synthetic_blob(0)), 1, 256)
        return R.build(name, table)[1], R.features(name, ROWS, FRAMES), 1, 10
    feats = np.stack([synthetic_features(3100 + b, FRAMES) for b in range(ROWS)])
    if name == "seed0":
        return synthetic_blob(0), feats, 1, 10
    if name == "skewed":
        return synthetic_blob(0, skew=0.1), feats, 2, 10
    if name == "slots12":
        return synthetic_blob(1), feats, 1, 12
    if name == "recur_first":
        return synthetic_blob(0, gru_a_order=GRUA_RECUR_FIRST), feats, 1, 10
    raise KeyError(name)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.nonzero(~(got.reshape(-1) == want.reshape(-1)))[0]
    assert not bad.size, (f"{what}: {bad.size} of {got.size} differ, first at {int(bad[0])}: kernel "
                          f"{got.reshape(-1)[int(bad[0])]!r} oracle {want.reshape(-1)[int(bad[0])]!r}")


@pytest.mark.parametrize("name", ["seed0", "hot", "tiny", "skewed", "slots12", "recur_first"])
def test_latency_kernel_against_the_oracle(oracle, name):
    from dss_amd import lpcnet
    from dss_amd.lpcnet import LPCNetBatch
    from dss_amd.nnet_data import kernel_fit
    blob, feats, fast_path, slots = _case(oracle, name)
    fit = kernel_fit(blob)
    assert (fit["fast_path"], fit["zr_register_slots"]) == (fast_path, slots), fit      # the instantiation this case is here for
    n, skip = FRAMES * 160, 320
    m = oracle.lpcnet_model(blob)
    exc = R.forced_excitation(ROWS, FRAMES)
    free, forced = [], []
    for b in range(ROWS):
        dec = oracle.decoder(m, trace_cap=n)
        pcm = np.concatenate([dec.synthesize(feats[b, t]) for t in range(FRAMES)])
        free.append((pcm, dec.trace_exc[:n - skip].copy(), dec.trace_pcm[:n - skip].copy()))
        dec = oracle.decoder(m, trace_cap=n)
        dec.force(exc[b, skip:])
        pcm = np.concatenate([dec.synthesize(feats[b, t]) for t in range(FRAMES)])
        assert np.isfinite(dec.forced_logits).all()
        forced.append((pcm, dec.forced_logits.copy(), dec.trace_pcm[:n - skip].copy()))
    try:
        lpcnet.load_model(blob)
        info = lpcnet.model_info()
        assert info["fast_path"] == fast_path and info["gru_a_order"] == (1 if name == "recur_first" else 0), info
        for trace in (False, True):                                            # free running
            gpu = LPCNetBatch(ROWS, FRAMES)
            gpu.set_multi(-1)
            if trace:
                gpu.enable_trace(1)
            pcm = gpu.synthesize(feats)
            for b in range(ROWS):
                tag = f"{name} / free running{' traced' if trace else ''} / row {b}"
                assert not pcm[b, :skip].any(), tag + ": silent frames"
                if trace:
                    _same(gpu.tap(b, 3, FRAMES).reshape(-1)[skip:].astype(np.uint8), free[b][1], tag + " / excitation")
                    _same(gpu.tap(b, 4, FRAMES).reshape(-1)[skip:], free[b][2], tag + " / pre-quantised value")
                _same(pcm[b], free[b][0], tag + " / PCM")
        gpu = LPCNetBatch(ROWS, FRAMES)                                        # teacher forced
        gpu.set_multi(-1)
        gpu.enable_trace(1)
        gpu.force_excitation(exc, FRAMES)
        pcm = gpu.synthesize(feats)
        for b in range(ROWS):
            tag = f"{name} / teacher forced / row {b}"
            _same(gpu.tap(b, 3, FRAMES).reshape(-1)[skip:].astype(np.uint8), exc[b, skip:], tag + " / excitation")
            _same(gpu.tap(b, 5, FRAMES).reshape(n, 256)[skip:], forced[b][1], tag + " / node logits (sample * 256 + node)")
            _same(gpu.tap(b, 4, FRAMES).reshape(-1)[skip:], forced[b][2], tag + " / pre-quantised value")
            _same(pcm[b], forced[b][0], tag + " / PCM")
    finally:
        lpcnet.load_model(synthetic_blob(0))
