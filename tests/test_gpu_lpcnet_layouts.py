"""GPU parity of the LPCNet sample-rate kernels against the CPU oracle on models that sit ON the capacity edges of the
CU-resident layout and one block past them (tests/lpcnet_layouts.py: register slots 8 / 10 / 12, tails of 16 and 17, h
slots 28 / 29 / 32 / 33 / 64 / 65, the image's spare records and over-reads, the pair kernel's and the LDS limit, sort
order, column order, a repeated column).  tests/test_cpu_lpcnet_layouts.py proves without a GPU that every case reaches
its edge.  Everything is compared with array_equal, tolerance 0.  Inputs: 3 rows x 5 frames, two silent frames plus 480
samples; the block lists run on every sample.

Compiled instantiations (sample_variants of lpcnet_sample.hip, pair_variants of lpcnet_sample_pair.hip; the phase-stamp
builds are diagnostic and stay out) and the case and call that runs each.  "Z = 10 plain" stands for the cases with
fast_path 1 and zr_cap 10 (z10, w03_8, h28, h_even, h_odd, h_none, h_wave_empty, h_overread, pair_last, pair_first_over,
lds_last, ties, descending_columns, repeated_column), "Z = 12" for z11, z12_r, z12x16, reversed and z12_order1, "extended"
for the cases with fast_path 2 (z13, w03_9, tail16_w45, tail16_w03, h29, h32, h33, h64, z13_order1).

  one-utterance kernel
    Z = 10 uniform          Z = 10 plain    test_free_running_every_kernel, automatic choice
    Z = 12 uniform          Z = 12          test_free_running_every_kernel, automatic choice
    Z = 10 ragged           Z = 10 plain    test_ragged_rows_and_carried_state, automatic choice
    Z = 12 ragged           Z = 12          test_ragged_rows_and_carried_state, automatic choice
    Z = 10 trace            Z = 10 plain    test_free_running_every_kernel traced; test_teacher_forced_logits
    Z = 12 trace            Z = 12          test_free_running_every_kernel traced; test_teacher_forced_logits
    extended uniform        extended        test_free_running_every_kernel, automatic choice
    extended ragged         extended        test_ragged_rows_and_carried_state, automatic choice
    extended trace          extended        test_free_running_every_kernel traced; test_teacher_forced_logits
    Z = 10 progressive      ties            test_progressive_call_equals_the_ragged_call
    Z = 12 progressive      z12_r           test_progressive_call_equals_the_ragged_call
    extended progressive    z13             test_progressive_call_equals_the_ragged_call
  pair kernel (set_multi(2); every case whose table entry says it fits)
    Z = 10 uniform          Z = 10 plain but pair_first_over, lds_last    test_free_running_every_kernel
    Z = 12 uniform          Z = 12          test_free_running_every_kernel
    Z = 10 trace            as above        test_free_running_every_kernel traced; test_teacher_forced_logits
    Z = 12 trace            Z = 12          test_free_running_every_kernel traced; test_teacher_forced_logits
    Z = 10 ragged           as above        test_ragged_rows_and_carried_state
    Z = 12 ragged           Z = 12          test_ragged_rows_and_carried_state
    Z = 10 ragged trace     as above        test_ragged_rows_and_carried_state traced
    Z = 12 ragged trace     Z = 12          test_ragged_rows_and_carried_state traced
  generic kernel            every case (enable_trace(16) / (17)); the automatic choice of tail17_w45, tail17_w03, h65, lds_first_over
"""
import warnings

import numpy as np
import pytest

import lpcnet_layouts as Y
import lpcnet_regimes as R
from dss_amd.lpcnet_weights import synthetic_blob

pytestmark = pytest.mark.gpu

_ref = {}


def _reference(oracle, name):
    """Oracle results of a case (computed once, read only): the model, and per row the free-running PCM, sampled excitation
    and pre-quantised value, and the teacher-forced PCM, node logits and pre-quantised value."""
    if name not in _ref:
        m = oracle.lpcnet_model(Y.build(name)[1])
        feats = Y.features()
        B, F = feats.shape[:2]
        n = (F - 2) * 160
        exc = R.forced_excitation(B, F)
        free, forced = [], []
        for b in range(B):
            dec = oracle.decoder(m, trace_cap=F * 160)
            pcm = np.concatenate([dec.synthesize(feats[b, t]) for t in range(F)])
            free.append((pcm, dec.trace_exc[:n].copy(), dec.trace_pcm[:n].copy()))
            dec = oracle.decoder(m, trace_cap=F * 160)
            dec.force(exc[b, 320:])
            pcm = np.concatenate([dec.synthesize(feats[b, t]) for t in range(F)])
            assert np.isfinite(dec.forced_logits).all()
            forced.append((pcm, dec.forced_logits.copy(), dec.trace_pcm[:n].copy()))
        _ref[name] = (m, feats, exc, free, forced)
    return _ref[name]


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
    """(label, set_multi, generic): the automatic choice on one utterance per workgroup, the generic kernel forced, the pair
    kernel where the table says the model fits."""
    ks = [("auto", -1, False), ("generic", -1, True)]
    if Y.CASES[name].pair_fits:
        ks.append(("pair", 2, False))
    return ks


def _load(name):
    from dss_amd import lpcnet
    c = Y.CASES[name]
    lpcnet.load_model(Y.build(name)[1])
    info = lpcnet.model_info()
    assert info["fast_path"] == c.fast_path and info["gru_a_order"] == c.gru_a_order, (name, info)
    return info


def _batch(name, rows, frames):
    """A decoder batch on the loaded model; the models beyond the outer capacities announce the generic kernel."""
    from dss_amd.lpcnet import LPCNetBatch
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        gpu = LPCNetBatch(rows, frames)
    loud = [x for x in seen if issubclass(x.category, RuntimeWarning) and "generic kernel" in str(x.message)]
    assert bool(loud) == (Y.CASES[name].fast_path == 0), (name, [str(x.message) for x in seen])
    return gpu


def _restore():
    from dss_amd import lpcnet
    lpcnet.load_model(synthetic_blob(0))


@pytest.mark.parametrize("name", list(Y.CASES))
def test_free_running_every_kernel(oracle, name):
    """int16 PCM of every row on the automatic choice, the forced generic kernel and, where it fits, the pair kernel; with
    trace also the sampled excitation and the pre-quantised value.  Where the table says the pair kernel does not fit,
    set_multi(2) is refused."""
    from dss_amd import _lib
    try:
        _load(name)
        _, feats, _, free, _ = _reference(oracle, name)
        B, F = feats.shape[:2]
        for label, multi, generic in _kernels(name):
            for trace in (False, True):
                gpu = _batch(name, B, F)
                gpu.set_multi(multi)
                if generic:
                    gpu.enable_trace(17 if trace else 16)
                elif trace:
                    gpu.enable_trace(1)
                pcm = gpu.synthesize(feats)
                for b in range(B):
                    tag = f"{name} / {label} kernel{' traced' if trace else ''} / row {b}"
                    if trace:
                        _same(gpu.tap(b, 3, F).reshape(-1)[320:].astype(np.uint8), free[b][1], tag + " / excitation")
                        _same(gpu.tap(b, 4, F).reshape(-1)[320:], free[b][2], tag + " / pre-quantised value")
                    _same(pcm[b], free[b][0], tag + " / PCM")
        if not Y.CASES[name].pair_fits:
            gpu = _batch(name, B, F)
            with pytest.raises(_lib.DssError, match="do not fit"):
                gpu.set_multi(2)
    finally:
        _restore()


@pytest.mark.parametrize("name", list(Y.CASES))
def test_teacher_forced_logits(oracle, name):
    """enable_trace(1) and a forced excitation (runs of 0 and of 255, swaps, noise): all 256 node logits of every sample, the
    pre-quantised value and the PCM, on the one-utterance kernel, the generic kernel and, where it fits, the pair kernel."""
    try:
        _load(name)
        _, feats, exc, _, forced = _reference(oracle, name)
        B, F = feats.shape[:2]
        n = F * 160
        for label, multi, generic in _kernels(name):
            gpu = _batch(name, B, F)
            gpu.set_multi(multi)
            gpu.enable_trace(17 if generic else 1)
            gpu.force_excitation(exc, F)
            pcm = gpu.synthesize(feats)
            for b in range(B):
                tag = f"{name} / {label} kernel / teacher forced / row {b}"
                _same(gpu.tap(b, 3, F).reshape(-1)[320:].astype(np.uint8), exc[b, 320:], tag + " / excitation")
                _same(gpu.tap(b, 5, F).reshape(n, 256)[320:], forced[b][1], tag + " / node logits (sample*256+node)")
                _same(gpu.tap(b, 4, F).reshape(-1)[320:], forced[b][2], tag + " / pre-quantised value")
                _same(pcm[b], forced[b][0], tag + " / PCM")
    finally:
        _restore()


@pytest.mark.parametrize("name", list(Y.CASES))
def test_ragged_rows_and_carried_state(oracle, name):
    """A ragged call with counts [5, 0, 3] whose slot list permutes the rows, then a second call on the carried state: the
    slot that ran 3 frames runs its last 2 (3 + 2 against 5 in one on the oracle), the one that ran none runs all 5.  On the
    one-utterance kernel and, where it fits, on the pair kernel, there also with trace (the ragged trace instantiation)."""
    calls = [[(2, 0, 5), (0, 0, 0), (1, 0, 3)],                  # (slot, first frame, frames), rows in this order
             [(1, 3, 2), (0, 0, 5), (2, 5, 0)]]
    try:
        _load(name)
        _, feats, _, free, _ = _reference(oracle, name)
        B, F = feats.shape[:2]
        for label, multi, generic in _kernels(name):
            if generic:
                continue
            for trace in ((False, True) if multi == 2 else (False,)):
                gpu = _batch(name, B, F)
                gpu.set_multi(multi)
                if trace:
                    gpu.enable_trace(1)
                for c, rows in enumerate(calls):
                    got = gpu.synthesize_ragged([feats[s, a:a + k] for s, a, k in rows], slots=[s for s, _, _ in rows],
                                                longest_first=False)
                    for (s, a, k), pcm in zip(rows, got):
                        _same(pcm, free[s][0][a * 160:(a + k) * 160],
                              f"{name} / {label} kernel{' traced' if trace else ''} / ragged call {c} / slot {s} frames {a}..{a + k}")
    finally:
        _restore()


@pytest.mark.parametrize("name", ["ties", "z12_r", "z13"])
def test_progressive_call_equals_the_ragged_call(name):
    """The progressive instantiations (10 slots, 12 slots, extended paths) deliver the ragged call's bytes."""
    from test_gpu_progressive import _ragged_against_progressive
    try:
        _load(name)
        _ragged_against_progressive()
    finally:
        _restore()


def test_automatic_choice_keeps_a_model_beyond_the_pair_limit_off_the_pair_kernel(oracle):
    """'pair_first_over' fits the one-utterance kernel but not the pair kernel.  A uniform call with more rows than the
    device has CUs, which the automatic rule gives to the pair kernel for a model that fits, runs and equals the oracle."""
    import torch
    from test_gpu_lpcnet import PAIR_RULE_ROWS as N_OVER_CUS
    name, F = "pair_first_over", 3
    assert N_OVER_CUS > max(128, torch.cuda.get_device_properties(0).multi_processor_count)      # the automatic rule's condition
    try:
        _load(name)
        m, feats, _, _, _ = _reference(oracle, name)
        dec = oracle.decoder(m)
        want = np.concatenate([dec.synthesize(feats[0, t]) for t in range(F)])
        gpu = _batch(name, N_OVER_CUS, F)
        pcm = gpu.synthesize(np.stack([feats[0, :F]] * N_OVER_CUS))
        _same(pcm[0], want, f"{name} / {N_OVER_CUS} rows / first row")
        _same(pcm[-1], want, f"{name} / {N_OVER_CUS} rows / last row")
        assert (pcm == pcm[0]).all()
    finally:
        _restore()
