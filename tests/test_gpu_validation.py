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

All of that is at the reference's sizes on decoder handles of 3, 4, 5 and 64 streams.  The tests named ``test_case_table_*`` run
the case table of tests/validation_cases.py (its conditions on the float64 reference alone: tests/test_cpu_validation.py).
Bounds, and beside them the worst figure measured on an MI355X over every entry:

* decoder, W = 2 and W = 4 chunks, chunks whose regressor blocks are pure padding or straddle a trial's end, O = 1, 3, 31, 32,
  K = 2H = 254 and 256, H = C = 1, float32 and float64 frames: every trial bit-identical to ``forward_rows_torch`` on a
  one-stream handle given that trial alone (so the handles of 300, 256 and 129 streams are bit-identical to each other),
  nothing written behind the last trial and no row left unwritten (the output holds a sentinel beforehand); features within
  ``bound(scale)`` = 2e-6 / 5e-5 of float64 on every trial: measured 1.05e-7 at scale 1 ((127, 255), 31 outputs; 4.98e-8 on the
  300-trial entry, 7.56e-8 at the reference size through ``decoder_validation``'s own handle), 9.34e-8 at scale 4;
* detector at (7, 5), (33, 17), (159, 127), (160, 128), (1, 1): bit-identical to ``step_torch`` per trial, labels equal to the
  float64 argmax on every frame (0 differences), logits within ``bound(scale)``: measured 4.17e-8 at scale 1 and 2.92e-7 at scale
  4, both at (160, 128); the tie model: labels all 0, prob exactly 0.5, |loss - ln 2| measured 0 (bound 1e-12);
* scores on synthetic logits (trials of 1, 255, 256, 257, 512, 513 frames, exp underflow, equal logits): a trial's loss within
  1e-12 x max(1, its largest per-frame cross-entropy) of numpy float64 (derived in ``test_case_table_scores``): measured 7.96e-13
  where the largest cross-entropy is 1600, i.e. 5.0e-4 of the bound, and 2.5e-16 where it is below 10; ``correct`` exact; prob
  within 1e-6: measured 2.97e-8, and exactly 0, 1 and 0.5 where it has to be; ``prob = NULL`` changes no bit;
* MSE with frames x outputs of 1, 255 ... 258, 279 elements: within 1e-12 relative of numpy float64: measured 2.15e-16 (4.35e-16
  on the 130 trials at the reference size); exactly 0.0 where the features are their targets.
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


# ---- the case table (tests/validation_cases.py) -------------------------------------------------------------------------------------
SENTINEL = 777.0
SPARE_ROWS = 8


def _cuda(x, f64):
    return torch.from_numpy(x if f64 else x.astype(np.float32)).cuda()


def _decoder_trials(k, x, ranges):
    """``dss_dec_forward_trials_dev`` into a tensor that holds SENTINEL beforehand and SPARE_ROWS rows more than the list fills: a
    row that is not written keeps the sentinel, and nothing may be written behind the last trial."""
    from dss_amd import _lib
    from dss_amd.validation import _ranges
    first, length, total = _ranges(k._L, int(x.shape[0]), ranges)
    feats = torch.full((total + SPARE_ROWS, k.O), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.check(k._L.dss_dec_forward_trials_dev(k._h, x.data_ptr(), int(x.dtype == torch.float64), int(x.shape[0]), len(first),
                                               first.ctypes.data, length.ctypes.data, feats.data_ptr(), torch.cuda.current_stream().cuda_stream))
    assert bool((feats[total:] == SENTINEL).all()), "rows behind the last trial were written"
    assert not bool((feats[:total] == SENTINEL).any()), "a row of the features was not written"
    return feats[:total]


def _detector_trials(k, x, ranges):
    """``dss_vad_forward_trials_dev`` into labels of -7 and logits of SENTINEL with SPARE_ROWS rows more than the list fills."""
    from dss_amd import _lib
    from dss_amd.validation import _ranges
    first, length, total = _ranges(k._L, int(x.shape[0]), ranges)
    labels = torch.full((total + SPARE_ROWS,), -7, dtype=torch.int32, device="cuda")
    logits = torch.full((total + SPARE_ROWS, 2), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.check(k._L.dss_vad_forward_trials_dev(k._h, x.data_ptr(), int(x.dtype == torch.float64), int(x.shape[0]), len(first),
                                               first.ctypes.data, length.ctypes.data, labels.data_ptr(), logits.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream))
    assert bool((labels[total:] == -7).all()) and bool((logits[total:] == SENTINEL).all()), "rows behind the last trial were written"
    assert bool(((labels[:total] == 0) | (labels[:total] == 1)).all()) and not bool((logits[:total] == SENTINEL).any())
    return labels[:total], logits[:total]


def _each_trial_alone(sd, x, ranges):
    """``forward_rows_torch`` on a ONE-stream handle, given each trial alone: the concatenated features in list order."""
    from dss_amd.decoder import BiLstmDecoderGPU
    k = BiLstmDecoderGPU(1, max(n for _, n in ranges), state_dict=sd)
    out = []
    for a, n in ranges:
        feats = torch.full((1, n, k.O), SENTINEL, dtype=torch.float32, device="cuda")
        out.append(k.forward_rows_torch(x[a:a + n][None].contiguous(), None, [n], feats, n)[0])
    return torch.cat(out)


def _trial_ids(lengths):
    return np.concatenate([np.full(n, (k % 3 + 1) * (-1) ** k, np.int16) for k, n in enumerate(lengths)])


def _first_difference(got, want, lengths):
    """The first trial (list position, length) in which two concatenated results differ in a bit, or None."""
    for k, s in enumerate(V.bounds_of(lengths)):
        if not torch.equal(_bits(got[s]), _bits(want[s])):
            return k, lengths[k]
    return None


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("e", [e for e in V.DECODER if not e.corpus_form], ids=V.dec_ident)
def test_case_table_decoder(e, f64):
    """Per decoder entry and handle: every trial of the trial form has the bits of ``forward_rows_torch`` on a one-stream handle
    given that trial alone (so W = 2 and W = 4 chunks, their partners taken from the longest-first order, equal single-trial
    calls, and the handles of 300, 256 and 129 streams equal each other); every feature within ``bound(scale)`` of the float64
    decoder, every trial of every entry compared; the output is written exactly where the list says."""
    from dss_amd.decoder import BiLstmDecoderGPU
    sd, x64, ranges = V.decoder_inputs(e)
    lengths = [n for _, n in ranges]
    x = _cuda(x64, f64)
    alone = _each_trial_alone(sd, x, ranges)
    truth = V.decoder_truth(e)
    want = np.concatenate([truth[i, :n] for i, n in enumerate(lengths)])
    for streams in e.handles:
        k = BiLstmDecoderGPU(streams, max(lengths), state_dict=sd)
        got = _decoder_trials(k, x, ranges)
        assert _first_difference(got, alone, lengths) is None, (streams, V.decoder_chunks(lengths, streams))
        assert torch.equal(_bits(k.forward_trials_torch(x, ranges)), _bits(got))
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print(f"{V.dec_ident(e)} f64={f64} handle of {streams} (chunks {V.decoder_chunks(lengths, streams)}): "
              f"|features - float64| {err:.2e} (bound {R.bound(e.scale):.0e})")
        assert err <= R.bound(e.scale)


@pytest.mark.parametrize("f64", [False, True])
def test_case_table_decoder_validation_at_the_reference_size(f64):
    """130 trials of 1 .. 12 frames at (100, 64) through ``decoder_validation(state_dict, ...)`` with ``max_streams`` left alone: the
    W = 2 chunk a corpus of more than 128 validation trials starts with.  Features bit-identical to single-trial calls and within
    bound of float64, the per-trial MSE within 1e-12 relative of numpy float64 on them."""
    from dss_amd.validation import decoder_validation
    e = V.REFERENCE_SIZE
    sd, x64, ranges = V.decoder_inputs(e)
    lengths = [n for _, n in ranges]
    assert [a for a, _ in ranges] == [int(v) for v in np.cumsum([0] + lengths[:-1])] and len(x64) == sum(lengths)
    frames = x64 if f64 else x64.astype(np.float32)
    tg = np.random.default_rng(9600).standard_normal((len(x64), e.O)).astype(np.float32)
    r = decoder_validation(sd, frames, tg, _trial_ids(lengths))
    feats = torch.from_numpy(r["features"]).cuda()
    assert _first_difference(feats, _each_trial_alone(sd, _cuda(x64, f64), ranges), lengths) is None
    truth = V.decoder_truth(e)
    got = r["features"].astype(np.float64)
    err = float(np.abs(got - np.concatenate([truth[i, :n] for i, n in enumerate(lengths)])).max())
    d = got - tg.astype(np.float64)
    want_mse = np.array([np.mean(d[s] ** 2) for s in V.bounds_of(lengths)])
    rel = float((np.abs(r["per_trial_mse"] - want_mse) / want_mse).max())
    print(f"reference size f64={f64}: |features - float64| {err:.2e} (bound {R.bound(e.scale):.0e}); largest relative |mse - numpy| {rel:.2e}")
    assert err <= R.bound(e.scale)
    assert (np.abs(r["per_trial_mse"] - want_mse) <= 1e-12 * want_mse).all() and r["loss"] == float(r["per_trial_mse"].mean())


def test_case_table_decoder_validation_sums():
    """``decoder_validation`` on an odd size, (33, 17) with one output: the features are the trial form's, ``per_trial_mse`` the
    reduction's on them, ``loss`` their mean; a state_dict and a handle the caller keeps agree bit for bit."""
    from dss_amd.decoder import BiLstmDecoderGPU
    from dss_amd.validation import decoder_validation
    e = V.DECODER_VALIDATION
    sd, x64, ranges = V.decoder_inputs(e)
    lengths = [n for _, n in ranges]
    cat = np.concatenate([x64[a:a + n] for a, n in ranges])
    tg = np.random.default_rng(9601).standard_normal((len(cat), e.O)).astype(np.float32)
    feats = _decoder_trials(BiLstmDecoderGPU(2, max(lengths), state_dict=sd), _cuda(x64, True), ranges)
    mse = _mse(feats, torch.from_numpy(tg).cuda(), lengths)
    d = feats.cpu().numpy().astype(np.float64) - tg.astype(np.float64)
    want = np.array([np.mean(d[s] ** 2) for s in V.bounds_of(lengths)])
    print(f"{V.dec_ident(e)}: largest relative |mse - numpy| {(np.abs(mse - want) / want).max():.2e}")
    assert (np.abs(mse - want) <= 1e-12 * want).all()
    ids = _trial_ids(lengths)
    for r in (decoder_validation(sd, cat, tg, ids), decoder_validation(sd, cat, tg, ids, max_streams=2),
              decoder_validation(BiLstmDecoderGPU(2, max(lengths), state_dict=sd), cat, tg, ids)):
        assert r["features"].shape == (len(cat), e.O) and np.array_equal(r["features"].view(np.int32), feats.cpu().numpy().view(np.int32))
        assert np.array_equal(r["per_trial_mse"], mse) and r["loss"] == float(mse.mean())


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("e", V.DETECTOR, ids=V.vad_ident)
def test_case_table_detector(e, f64):
    """Per detector entry: every trial of the trial form has the bits of ``step_torch`` on a fresh one-stream handle; logits
    within ``bound(scale)`` of the float64 detector; labels equal to its argmax on EVERY frame (the entries have no near-tie:
    tests/test_cpu_validation.py::test_case_table_detector_has_no_near_tie)."""
    from dss_amd.vad import VadLstmGPU
    sd, x64, ranges = V.detector_inputs(e)
    x = _cuda(x64, f64)
    labels, logits = _detector_trials(VadLstmGPU(2, state_dict=sd), x, ranges)
    for (a, n), s in zip(ranges, V.bounds_of(e.lengths)):
        lab, lg = VadLstmGPU(1, state_dict=sd).step_torch(x[None, a:a + n], want_logits=True)
        assert torch.equal(_bits(logits[s]), _bits(lg[0])), f"trial ({a}, {n}): logits differ from the streaming form"
        assert torch.equal(labels[s], lab[0]), f"trial ({a}, {n}): labels differ from the streaming form"
    want = V.detector_truth(e)
    err = float(np.abs(logits.cpu().numpy().astype(np.float64) - want).max())
    differ = int((labels.cpu().numpy() != (want[:, 1] > want[:, 0])).sum())
    print(f"{V.vad_ident(e)} f64={f64}: |logits - float64| {err:.2e} (bound {R.bound(e.scale):.0e}); label differences {differ} of {len(want)}")
    assert err <= R.bound(e.scale)
    assert differ == 0


def test_case_table_tie_model():
    """Equal classifier rows: every logit pair equal bit for bit, so every label 0 (the first maximum wins), prob exactly 0.5
    and a loss of ln 2 on every frame -- each frame scored as a trial of its own, against both targets."""
    from dss_amd.vad import VadLstmGPU
    sd, x64, ranges = V.detector_inputs(V.TIE)
    labels, logits = _detector_trials(VadLstmGPU(2, state_dict=sd), _cuda(x64, False), ranges)
    z = logits.cpu().numpy()
    assert np.array_equal(z[:, 0].view(np.int32), z[:, 1].view(np.int32)) and np.ptp(z[:, 0]) > 0
    assert not labels.cpu().numpy().any()
    want = V.detector_truth(V.TIE)
    print(f"tie model: |logits - float64| {np.abs(z - want).max():.2e} (bound {R.bound(1):.0e})")
    assert np.abs(z - want).max() <= R.bound(1)
    n = len(z)
    for tg in (np.zeros(n, np.uint8), np.ones(n, np.uint8)):
        loss, correct, prob = _score(logits, labels, tg, [1] * n)
        print(f"tie model, targets {int(tg[0])}: largest |loss - ln 2| {np.abs(loss - np.log(2.0)).max():.2e}")
        assert np.array_equal(prob, np.full(n, 0.5, np.float32))
        assert np.abs(loss - np.log(2.0)).max() <= 1e-12
        assert np.array_equal(correct, 1 - tg.astype(np.int32))


def test_case_table_detector_validation_sums():
    """``vad_validation`` on an odd size, (33, 17): ``loss`` is the sum and ``accuracy`` the ratio of the per-trial figures, which
    are the reduction's on the trial form's logits; a state_dict and a handle the caller keeps agree bit for bit."""
    from dss_amd.vad import VadLstmGPU
    from dss_amd.validation import vad_validation
    e = V.DETECTOR_VALIDATION
    sd, x64, ranges = V.detector_inputs(e)
    lengths = list(e.lengths)
    cat = np.concatenate([x64[a:a + n] for a, n in ranges])
    tg = np.resize(np.array([0, 0, 1, 1, 1], np.uint8), len(cat))
    labels, logits = _detector_trials(VadLstmGPU(1, state_dict=sd), _cuda(x64, True), ranges)
    loss, correct, prob = _score(logits, labels, tg, lengths)
    ce = V.cross_entropy(logits.cpu().numpy(), tg)
    want = np.array([ce[s].mean() for s in V.bounds_of(lengths)])
    print(f"{V.vad_ident(e)}: largest |loss - numpy| {np.abs(loss - want).max():.2e}, largest per-frame cross-entropy {ce.max():.3f}")
    assert np.abs(loss - want).max() <= 1e-12 * max(1.0, ce.max())
    lab = labels.cpu().numpy()
    assert np.array_equal(correct, [int((lab[s] == tg[s]).sum()) for s in V.bounds_of(lengths)])
    ids = _trial_ids(lengths)
    for r in (vad_validation(sd, cat, tg, ids), vad_validation(VadLstmGPU(3, state_dict=sd), cat, tg.astype(bool), ids)):
        assert np.array_equal(r["per_trial_loss"], loss) and np.array_equal(r["per_trial_correct"], correct)
        assert np.array_equal(r["pred"], lab) and np.array_equal(r["prob"], prob)
        assert r["loss"] == float(loss.sum()) and r["accuracy"] == float(correct.sum()) / len(cat)


def test_case_table_scores():
    """``dss_vad_score_trials_dev`` on synthetic float32 logits: trials of 1, 255, 256, 257, 512 and 513 frames (its tile is 256
    frames); N(0, 3) logits mixed with runs where exp(z - m) underflows and runs of equal logits; targets equal to the strict
    argmax, to its complement, and in runs against every kind of frame; labels the argmax and its complement.

    The bound on a trial's loss against numpy float64 on the same logits is 1e-12 x max(1, the trial's largest per-frame
    cross-entropy).  It is derived, not measured: a sequential float64 sum of L <= 513 terms is off by at most L x 2^-53 x sum|ce|,
    which after the division by L is under 513 x 1.1e-16 = 6e-14 times the largest term, and numpy's own mean is at least as
    close; device and host ``log`` / ``exp`` differ by a few ulp (2.2e-16 relative) of each term, and the sum m + log(.) rounds
    once more at the size of the result.  All of that is below 1e-13 x max(1, max ce); the bound leaves a factor of ten.
    ``correct`` is exact; ``prob`` is within 1e-6 of the float64 softmax (it is a float32: 6e-8 relative), exactly 0.0 / 1.0
    where the other logit's exp underflows and exactly 0.5 on equal logits (exp(-ln 2 (1 + a few 1e-16)) rounds to 0.5 in float32).
    With ``prob = NULL`` the other results are the same bits."""
    z, kind, argmax, runs = V.score_inputs()
    lengths = list(V.SCORE_LENGTHS)
    sl = V.bounds_of(lengths)
    logits = torch.from_numpy(z).cuda()
    soft = V.softmax_speech(z)
    worst = worst_prob = 0.0
    for tname, tg in (("argmax", argmax.astype(np.uint8)), ("complement", (1 - argmax).astype(np.uint8)), ("runs", runs)):
        ce = V.cross_entropy(z, tg)
        want = np.array([ce[s].mean() for s in sl])
        bound = np.array([1e-12 * max(1.0, ce[s].max()) for s in sl])
        for lname, lab in (("argmax", argmax), ("complement", 1 - argmax)):
            labels = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).cuda()
            loss, correct, prob = _score(logits, labels, tg, lengths)
            loss_np, correct_np, _ = _score(logits, labels, tg, lengths, want_prob=False)
            assert np.array_equal(loss.view(np.int64), loss_np.view(np.int64)) and np.array_equal(correct, correct_np)
            ratio = float((np.abs(loss - want) / bound).max())
            print(f"targets {tname}, labels {lname}: |loss - numpy| {np.abs(loss - want).max():.2e}, at most {ratio:.1e} of a trial's bound; "
                  f"|prob - softmax| {np.abs(prob - soft).max():.2e}; correct {correct.tolist()}")
            worst, worst_prob = max(worst, ratio), max(worst_prob, float(np.abs(prob - soft).max()))
            assert (np.abs(loss - want) <= bound).all()
            assert np.array_equal(correct, [int((lab[s] == tg[s]).sum()) for s in sl])
            if tname == "argmax":
                assert np.array_equal(correct, lengths if lname == "argmax" else [0] * len(lengths))
            assert np.abs(prob - soft).max() <= 1e-6
            assert np.array_equal(prob[kind == 1], np.zeros((kind == 1).sum(), np.float32))
            assert np.array_equal(prob[kind == 2], np.ones((kind == 2).sum(), np.float32))
            assert np.array_equal(prob[kind == 3], np.full((kind == 3).sum(), 0.5, np.float32))
        if tname != "runs":          # loss 0 / the whole gap on the underflow runs
            under = (kind == 1) | (kind == 2)
            assert set(np.unique(ce[under])) == ({0.0} if tname == "argmax" else {2.0 * V.UNDERFLOW})
    print(f"scores: worst |loss - numpy| / bound {worst:.1e}, worst |prob - softmax| {worst_prob:.2e}")


@pytest.mark.parametrize("frames,outputs", V.MSE_CASES)
def test_case_table_mse(frames, outputs):
    """``dss_dec_mse_trials_dev`` with frames x outputs on either side of the kernel's stride of 256 elements, between two short
    trials: within 1e-12 relative of numpy float64, and exactly 0.0 where the features are their targets bit for bit."""
    lengths, feats, tg = V.mse_inputs(frames, outputs)
    f, t = torch.from_numpy(feats).cuda(), torch.from_numpy(tg).cuda()
    mse = _mse(f, t, lengths)
    d = feats.astype(np.float64) - tg.astype(np.float64)
    want = np.array([np.mean(d[s] ** 2) for s in V.bounds_of(lengths)])
    print(f"({frames}, {outputs}): largest relative |mse - numpy| {(np.abs(mse - want) / want).max():.2e}")
    assert (np.abs(mse - want) <= 1e-12 * want).all()
    zero = _mse(f, f.clone(), lengths)
    assert np.array_equal(zero, np.zeros(len(lengths))) and not np.signbit(zero).any()
