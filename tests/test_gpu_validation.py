"""The two recurrent models over a trial list (Part 8 of include/dss_hip.h; dss_amd/validation.py) on the GPU.

* the trial form is the streaming / ragged form bit for bit: every trial of ``VadLstmGPU.forward_trials_torch`` against
  ``step_torch`` on a fresh one-stream handle, every trial of ``BiLstmDecoderGPU.forward_trials_torch`` against
  ``forward_rows_torch`` -- lengths 1, 3, 4, 5, 50, 251, 1500, overlapping ranges, more trials than the handle has streams;
* a trial-list call leaves the detector's streaming state alone;
* logits and features within ``lstm_reference.bound(scale)`` of the float64 models, labels equal on EVERY frame (the corpus has
  no near-tie: tests/test_cpu_validation.py::test_fixture_has_no_near_tie);
* the scores: per-trial cross-entropy within 2 x bound + 1e-12 of the float64 model's (cross-entropy is 2-Lipschitz in the
  logits' sup norm) and within 1e-12 of numpy float64 on the returned logits, the correct count exact, prob within 1e-6, the
  per-trial MSE within 1e-12 relative of numpy float64 on the returned features; ``vad_validation`` / ``decoder_validation``
  return their sum / ratio / mean.
Every figure is printed before it is asserted (run with -rP)."""
import numpy as np
import pytest
import torch

import lstm_reference as R
import validation_cases as V

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(torch.get_num_threads(), 16))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _frames(scale, f64):
    x = V.corpus(scale)
    return torch.from_numpy(x if f64 else x.astype(np.float32)).cuda()


def _score(logits, labels, targets, lengths, want_prob=True):
    from dss_amd import _lib
    L = _lib.require_gpu()
    n = len(lengths)
    length = np.ascontiguousarray(lengths, dtype=np.int32)
    loss = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    correct = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    prob = torch.full((int(length.sum()),), -1.0, dtype=torch.float32, device="cuda") if want_prob else None
    tg = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.uint8)).cuda()
    _lib.check(L.dss_vad_score_trials_dev(logits.data_ptr(), labels.data_ptr(), tg.data_ptr(), n, length.ctypes.data, loss.data_ptr(),
                                          correct.data_ptr(), prob.data_ptr() if want_prob else None,
                                          torch.cuda.current_stream().cuda_stream))
    return loss.cpu().numpy(), correct.cpu().numpy(), prob.cpu().numpy() if want_prob else None


def _mse(feats, targets, lengths):
    from dss_amd import _lib
    L = _lib.require_gpu()
    n = len(lengths)
    length = np.ascontiguousarray(lengths, dtype=np.int32)
    out = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
    _lib.check(L.dss_dec_mse_trials_dev(feats.data_ptr(), targets.data_ptr(), int(feats.shape[1]), n, length.ctypes.data, out.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy()


# ---- detector ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True])
def test_vad_trials_bit_identical_to_streaming(f64):
    """Ten trials on a handle of TWO streams, against step_torch on a fresh one-stream handle given each trial alone."""
    from dss_amd.vad import VadLstmGPU
    sd = R.vad_state_dict(V.VAD_H, V.C, 4)
    x = _frames(4, f64)
    labels, logits = VadLstmGPU(2, state_dict=sd).forward_trials_torch(x, V.RANGES, want_logits=True)
    only_labels = VadLstmGPU(2, state_dict=sd).forward_trials_torch(x, V.RANGES)
    assert labels.dtype == torch.int32 and logits.dtype == torch.float32 and logits.shape == (labels.shape[0], 2)
    assert torch.equal(labels, only_labels)
    for (a, n), sl in zip(V.RANGES, V.trial_slices()):
        lab, lg = VadLstmGPU(1, state_dict=sd).step_torch(x[None, a:a + n], want_logits=True)
        assert torch.equal(_bits(logits[sl]), _bits(lg[0])), f"trial ({a}, {n}): logits differ from the streaming form"
        assert torch.equal(labels[sl], lab[0]), f"trial ({a}, {n}): labels differ from the streaming form"
    assert 0.05 < float(labels.float().mean()) < 0.95      # both classes occur


def test_vad_trials_many_short_trials():
    """300 trials (more than one reduction launch takes) of 1 .. 9 frames at random rows, in list order whatever their lengths."""
    from dss_amd.vad import VadLstmGPU
    sd = R.vad_state_dict(V.VAD_H, V.C, 4)
    x = _frames(4, False)
    rng = np.random.default_rng(31)
    ranges = [(int(rng.integers(0, V.N_ROWS - 9)), int(rng.integers(1, 10))) for _ in range(300)]
    labels, logits = VadLstmGPU(1, state_dict=sd).forward_trials_torch(x, ranges, want_logits=True)
    b = np.concatenate([[0], np.cumsum([n for _, n in ranges])])
    for k in (0, 1, 149, 255, 256, 257, 299):
        a, n = ranges[k]
        lab, lg = VadLstmGPU(1, state_dict=sd).step_torch(x[None, a:a + n], want_logits=True)
        assert torch.equal(_bits(logits[b[k]:b[k + 1]]), _bits(lg[0])) and torch.equal(labels[b[k]:b[k + 1]], lab[0]), k
    tg = rng.integers(0, 2, int(b[-1])).astype(np.uint8)
    loss, correct, _ = _score(logits, labels, tg, [n for _, n in ranges])
    z, lab = logits.cpu().numpy(), labels.cpu().numpy()
    ce = V.cross_entropy(z, tg)
    want = np.array([ce[b[k]:b[k + 1]].mean() for k in range(300)])
    print("300 trials: largest |loss - numpy|", np.abs(loss - want).max())
    assert np.abs(loss - want).max() <= 1e-12
    assert np.array_equal(correct, [int((lab[b[k]:b[k + 1]] == tg[b[k]:b[k + 1]]).sum()) for k in range(300)])


def test_vad_trials_leave_the_streaming_state_alone():
    """step -> forward_trials -> step equals step -> step, bit for bit, state() included."""
    from dss_amd.vad import VadLstmGPU
    sd = R.vad_state_dict(V.VAD_H, V.C, 4)
    x = _frames(4, False)
    p1, p2 = x[:8].reshape(2, 4, V.C), x[8:18].reshape(2, 5, V.C)
    a, b = VadLstmGPU(2, state_dict=sd), VadLstmGPU(2, state_dict=sd)
    a1 = a.step_torch(p1, want_logits=True)
    a.forward_trials_torch(x, V.RANGES, want_logits=True)
    ha, ca = a.state()
    a2 = a.step_torch(p2, want_logits=True)
    b1 = b.step_torch(p1, want_logits=True)
    hb, cb = b.state()
    b2 = b.step_torch(p2, want_logits=True)
    assert np.array_equal(ha.view(np.int32), hb.view(np.int32)) and np.array_equal(ca.view(np.int32), cb.view(np.int32))
    assert np.abs(ha).max() > 0
    for got, want in ((a1, b1), (a2, b2)):
        assert torch.equal(got[0], want[0]) and torch.equal(_bits(got[1]), _bits(want[1]))
    for got, want in zip(a.state(), b.state()):
        assert np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("scale", [1, 4])
def test_vad_trials_against_float64_and_scores(scale):
    from dss_amd.vad import VadLstmGPU
    from dss_amd.validation import vad_validation
    sd = R.vad_state_dict(V.VAD_H, V.C, scale)
    x = _frames(scale, scale == 4)
    labels, logits = VadLstmGPU(3, state_dict=sd).forward_trials_torch(x, V.RANGES, want_logits=True)
    z, lab = logits.cpu().numpy().astype(np.float64), labels.cpu().numpy()
    want = V.vad_reference_logits(scale)
    err = float(np.abs(z - want).max())
    print(f"x{scale}: |logits - float64| {err:.2e} (bound {R.bound(scale):.0e}); label differences "
          f"{int((lab != (want[:, 1] > want[:, 0])).sum())} of {len(lab)}")
    assert err <= R.bound(scale)
    assert np.array_equal(lab, (want[:, 1] > want[:, 0]).astype(np.int32))          # every frame: the corpus has no near-tie

    tg = V.targets(scale)
    lengths = [n for _, n in V.RANGES]
    loss, correct, prob = _score(logits, labels, tg, lengths)
    loss_np, correct_np, _ = _score(logits, labels, tg, lengths, want_prob=False)
    assert np.array_equal(loss, loss_np) and np.array_equal(correct, correct_np)
    ce_ref, ce_got = V.cross_entropy(want, tg), V.cross_entropy(z, tg)
    sl = V.trial_slices()
    ref = np.array([ce_ref[s].mean() for s in sl])
    got = np.array([ce_got[s].mean() for s in sl])
    print(f"x{scale}: |loss - float64 model| {np.abs(loss - ref).max():.2e}; |loss - numpy on the logits| {np.abs(loss - got).max():.2e}")
    assert np.abs(loss - ref).max() <= 2 * R.bound(scale) + 1e-12
    assert np.abs(loss - got).max() <= 1e-12
    assert np.array_equal(correct, [int((lab[s] == tg[s]).sum()) for s in sl])
    soft = 1.0 / (1.0 + np.exp(z[:, 0] - z[:, 1]))
    print(f"x{scale}: |prob - float64 softmax| {np.abs(prob - soft).max():.2e}")
    assert np.abs(prob - soft).max() <= 1e-6

    # the corpus form: the trials' frames concatenated, cut by trial_ids, behind a 128 -> 64 channel gather
    xc = V.corpus(scale)
    cat = np.concatenate([xc[a:a + n] for a, n in V.RANGES])
    ids = np.concatenate([np.full(n, (k % 3 + 1) * (-1) ** k, np.int16) for k, n in enumerate(lengths)])
    cols = np.random.default_rng(5).permutation(128)[:64]
    wide = np.random.default_rng(6).standard_normal((len(cat), 128))
    wide[:, cols] = cat
    for r in (vad_validation(sd, cat, tg.astype(bool), ids), vad_validation(sd, wide, tg, ids, columns=cols),
              vad_validation(VadLstmGPU(2, state_dict=sd), cat, tg, ids)):          # a handle the caller keeps
        assert np.array_equal(r["per_trial_loss"], loss) and np.array_equal(r["per_trial_correct"], correct)
        assert np.array_equal(r["pred"], lab) and np.array_equal(r["prob"], prob)
        assert r["loss"] == float(loss.sum()) and r["accuracy"] == float(correct.sum()) / len(lab)
        assert r["pred"].dtype == np.int32 and r["prob"].dtype == np.float32 and r["per_trial_loss"].dtype == np.float64


# ---- decoder ----------------------------------------------------------------------------------------------------------------
def _rows_form(sd, x, ranges, T):
    """forward_rows_torch on the same trials: one pool row per trial."""
    from dss_amd.decoder import BiLstmDecoderGPU
    n = len(ranges)
    pool = torch.zeros((n, T, x.shape[1]), dtype=x.dtype, device="cuda")
    for i, (a, m) in enumerate(ranges):
        pool[i, :m] = x[a:a + m]
    feats = torch.full((n, T, 20), 777.0, dtype=torch.float32, device="cuda")
    BiLstmDecoderGPU(n, T, state_dict=sd).forward_rows_torch(pool, None, [m for _, m in ranges], feats, T)
    return feats


@pytest.mark.parametrize("f64", [False, True])
def test_decoder_trials_bit_identical_to_rows(f64):
    """Ten trials on a handle of FOUR streams (three chunks inside the call) against forward_rows on a handle that takes all."""
    from dss_amd.decoder import BiLstmDecoderGPU
    sd = R.decoder_state_dict(V.DEC_H, V.C, 4)
    x = _frames(4, f64)
    got = BiLstmDecoderGPU(4, 1500, state_dict=sd).forward_trials_torch(x, V.RANGES)
    assert got.shape == (sum(n for _, n in V.RANGES), 20) and got.dtype == torch.float32
    rows = _rows_form(sd, x, V.RANGES, 1500)
    for i, ((a, n), sl) in enumerate(zip(V.RANGES, V.trial_slices())):
        assert torch.equal(_bits(got[sl]), _bits(rows[i, :n])), f"trial ({a}, {n}) differs from forward_rows"


def test_decoder_trials_many_short_trials_and_mse():
    """300 trials of 1 .. 9 frames on a handle of 64 streams (five chunks), against forward_rows on a handle of 300."""
    from dss_amd.decoder import BiLstmDecoderGPU
    sd = R.decoder_state_dict(V.DEC_H, V.C, 1)
    x = _frames(1, False)
    rng = np.random.default_rng(32)
    ranges = [(int(rng.integers(0, V.N_ROWS - 9)), int(rng.integers(1, 10))) for _ in range(300)]
    got = BiLstmDecoderGPU(64, 9, state_dict=sd).forward_trials_torch(x, ranges)
    rows = _rows_form(sd, x, ranges, 9)
    b = np.concatenate([[0], np.cumsum([n for _, n in ranges])])
    for k, (_, n) in enumerate(ranges):
        assert torch.equal(_bits(got[b[k]:b[k + 1]]), _bits(rows[k, :n])), k
    tg = torch.from_numpy(rng.standard_normal((int(b[-1]), 20)).astype(np.float32)).cuda()
    mse = _mse(got, tg, [n for _, n in ranges])
    d = got.cpu().numpy().astype(np.float64) - tg.cpu().numpy().astype(np.float64)
    want = np.array([np.mean(d[b[k]:b[k + 1]] ** 2) for k in range(300)])
    print("300 trials: largest relative |mse - numpy|", (np.abs(mse - want) / want).max())
    assert (np.abs(mse - want) <= 1e-12 * want).all()


def test_decoder_trial_longer_than_max_frames_raises():
    from dss_amd import _lib
    from dss_amd.decoder import BiLstmDecoderGPU
    sd = R.decoder_state_dict(V.DEC_H, V.C, 1)
    x = _frames(1, False)
    k = BiLstmDecoderGPU(4, 250, state_dict=sd)
    with pytest.raises(_lib.DssError, match="max_frames"):
        k.forward_trials_torch(x, [(0, 50), (100, 251)])
    with pytest.raises(_lib.DssError):
        k.forward_trials_torch(x, [(V.N_ROWS - 3, 4)])
    assert k.forward_trials_torch(x, [(0, 250)]).shape == (250, 20)


@pytest.mark.parametrize("scale", [1, 4])
def test_decoder_trials_against_float64_and_mse(scale):
    from dss_amd.decoder import BiLstmDecoderGPU
    from dss_amd.validation import decoder_validation
    sd = R.decoder_state_dict(V.DEC_H, V.C, scale)
    xc = V.corpus(scale)
    x = _frames(scale, scale == 1)
    feats = BiLstmDecoderGPU(4, 1500, state_dict=sd).forward_trials_torch(x, V.RANGES)
    got = feats.cpu().numpy().astype(np.float64)
    lengths = [n for _, n in V.RANGES]
    pool = np.zeros((len(V.RANGES), 1500, V.C))
    for i, (a, n) in enumerate(V.RANGES):
        pool[i, :n] = xc[a:a + n]
    ref, _ = R.decoder_forward(R.Net(sd), pool, lengths=lengths)
    want = np.concatenate([ref[i, :n] for i, n in enumerate(lengths)])
    err = float(np.abs(got - want).max())
    print(f"x{scale}: |features - float64| {err:.2e} (bound {R.bound(scale):.0e})")
    assert err <= R.bound(scale)

    tg = V.lpc_targets(scale)
    mse = _mse(feats, torch.from_numpy(tg).cuda(), lengths)
    d = got - tg.astype(np.float64)
    want_mse = np.array([np.mean(d[s] ** 2) for s in V.trial_slices()])
    print(f"x{scale}: largest relative |mse - numpy| {(np.abs(mse - want_mse) / want_mse).max():.2e}")
    assert (np.abs(mse - want_mse) <= 1e-12 * want_mse).all()

    cat = np.concatenate([xc[a:a + n] for a, n in V.RANGES])
    ids = np.concatenate([np.full(n, (k % 3 + 1) * (-1) ** k, np.int16) for k, n in enumerate(lengths)])
    for r in (decoder_validation(sd, cat, tg, ids), decoder_validation(sd, cat, tg, ids, max_streams=3),
              decoder_validation(BiLstmDecoderGPU(5, 1500, state_dict=sd), cat, tg, ids)):          # a handle the caller keeps
        assert np.array_equal(r["features"].view(np.int32), feats.cpu().numpy().view(np.int32))
        assert np.array_equal(r["per_trial_mse"], mse) and r["loss"] == float(mse.mean())
