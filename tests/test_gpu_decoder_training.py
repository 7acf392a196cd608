"""The decoder's training step on the GPU (csrc/dec_train.hip, dss_amd/training.py) against the float64 references of
tests/decoder_training_reference.py: gradients, loss and features per trial; the RMSprop update against the float64 formula on the
kernel's own read-back values; publish; determinism; the forward half against the inference kernel, bit for bit; learning.

Bounds: gradients D.GRAD_BOUND per tensor (max|g - g64| / max|g64|; 4 x torch float32 CPU autograd's own error, see the helper);
features lstm_reference.bound(scale), the inference kernel's bound, which the forward half shares with its arithmetic; the loss
from that bound (see ``D.loss_bound``)."""
import numpy as np
import pytest

import lstm_reference as R
import decoder_training_reference as D
import training_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    from dss_amd import training
    return training


def _check_trial(*args, **kw):
    """The checker lives in the helper module (tests/test_gpu_training_cases.py runs it too); the worst gradient error."""
    return D.check_trial(*args, **kw)[0]


@pytest.mark.parametrize("case", D.GRAD_CASES, ids=str)
def test_gradients_loss_and_features_against_float64(T, case):
    worst = 0.0
    tr = None
    long = case[2] >= 350                                  # the real trial length runs once: with a mask, float32 frames
    for mask in (("random",) if long else (None, "random")):
        sd, x, y, m = D.case_inputs(case, mask)
        tr = tr or T.DecoderTrainerGPU(sd, max_frames=case[2])
        want = D.autograd_trial(sd, x, y, m)
        for f64 in ((False,) if long else (False, True)):
            worst = max(worst, _check_trial(tr, sd, x, y, m, case[3], f64, f"{case} mask={mask} f64={f64}", want))
    print(f"{case}: worst gradient error {worst:.3g} (bound {D.GRAD_BOUND:g})")


def test_mask_with_an_all_zero_row(T):
    case = D.GRAD_CASES[6]
    sd, x, y, m = D.case_inputs(case, "zero_row")
    assert not m[case[2] // 2].any()
    _check_trial(T.DecoderTrainerGPU(sd, max_frames=64), sd, x, y, m, 1, False, f"{case} mask=zero_row")


def test_trial_sizes_are_checked(T):
    from dss_amd import _lib
    sd, x, y, m = D.case_inputs(D.GRAD_CASES[5], None)
    tr = T.DecoderTrainerGPU(sd, max_frames=4)
    with pytest.raises(_lib.DssError, match="trial of 7"):
        tr.trial(x, y)
    with pytest.raises(ValueError, match="mask must be"):
        T.DecoderTrainerGPU(sd, max_frames=8).trial(x, y, mask=np.zeros((7, 6), np.float32))


def _ulp32(v):
    v = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


@pytest.mark.parametrize("case", (D.GRAD_CASES[6], D.GRAD_CASES[5]) + TC.RMSPROP_CASES, ids=str)
def test_rmsprop_update_is_the_float64_formula(T, case):
    """Two consecutive steps (the first from sq = 0): p', sq' against the float64 formula on the read-back float32 p, sq and the
    kernel's own g, with the detector test's bounds (sq: 4 x 2^-24 relative; p: one ulp + 4 x 2^-24 |dp|); bias_ih / bias_hh: equal
    g, separate updates; step=False leaves p and sq bit-identical."""
    sd, x, y, m = D.case_inputs(case, "random")
    tr = T.DecoderTrainerGPU(sd, max_frames=64)
    lr, alpha, eps = 1e-3, 0.99, 1e-8
    u = 2.0 ** -24
    for step in range(2):
        p0, s0 = tr.state_dict(), tr.square_avg()
        tr.trial(x, y, mask=m, step=False)
        assert all(np.array_equal(p0[k].numpy(), tr.state_dict()[k].numpy()) for k in D.KEYS)
        assert all(np.array_equal(s0[k], tr.square_avg()[k]) for k in D.KEYS)
        tr.trial(x, y, mask=m, step=True, lr=lr, alpha=alpha, eps=eps)
        g, p1, s1 = tr.gradients(), tr.state_dict(), tr.square_avg()
        if step == 0:
            assert all(not s0[k].any() for k in D.KEYS)
        for k in D.KEYS:
            pw, sw = D.rmsprop64(p0[k].numpy(), s0[k], g[k], lr, alpha, eps)
            assert (np.abs(s1[k] - sw) <= 4 * u * sw).all(), (step, k)
            dp = np.abs(pw - p0[k].numpy().astype(np.float64))
            assert (np.abs(p1[k].numpy() - pw) <= _ulp32(pw) + 4 * u * dp).all(), (step, k)
            assert np.abs(dp).max() > 0
        for layer in (0, 1):
            for rev in ("", "_reverse"):
                bi, bh = f"lstm.bias_ih_l{layer}{rev}", f"lstm.bias_hh_l{layer}{rev}"
                assert np.array_equal(g[bi], g[bh])
                if step == 1:  # the two biases started apart, so equal g moved them by the same formula from different p
                    assert not np.array_equal(p1[bi].numpy(), p1[bh].numpy())


def test_publish_is_loading_the_state_dict(T):
    """The packed copies follow the master parameters: a published handle computes, bit for bit, what a handle loaded from
    state_dict() computes, and not what the initial weights give."""
    import torch
    from dss_amd.decoder import BiLstmDecoderGPU
    case = D.GRAD_CASES[6]
    sd, x, y, m = D.case_inputs(case, "random")
    tr = T.DecoderTrainerGPU(sd, max_frames=64)
    for _ in range(2):
        tr.trial(x, y, mask=m, step=True, lr=1e-3)
    dec = BiLstmDecoderGPU(1, 64, state_dict=sd)
    xs = torch.from_numpy(x.astype(np.float32)).cuda()[None]
    before = dec(xs).clone()
    tr.publish(dec)
    got = dec(xs)
    want = BiLstmDecoderGPU(1, 64, state_dict=tr.state_dict())(xs)
    assert torch.equal(got, want)
    assert not torch.equal(got, before)
    with pytest.raises(Exception, match="inputs"):
        tr.publish(BiLstmDecoderGPU(1, 64, state_dict=R.decoder_state_dict(16, 8, 1)))


@pytest.mark.parametrize("H, C, n", [(16, 8, 120), (100, 64, 101)])
def test_the_same_trial_twice_gives_the_same_bits(T, H, C, n):
    sd = R.decoder_state_dict(H, C, 1)
    x = R.frames("x2", 1, n, C, 31 * n + H)[0]
    rng = np.random.default_rng(n + H)
    y = rng.standard_normal((n, 20)).astype(np.float32)
    mask = (rng.random((n, 2 * H)) >= 0.5).astype(np.float32) * np.float32(2.0)
    runs = []
    for _ in range(2):
        tr = T.DecoderTrainerGPU(sd, max_frames=128)
        losses = [tr.trial(x, y, mask=mask, step=True, lr=1e-3) for _ in range(2)]
        runs.append((losses, tr.state_dict(), tr.square_avg(), tr.gradients()))
    assert runs[0][0] == runs[1][0]
    for k in D.KEYS:
        for j in (1, 2, 3):
            a, b = runs[0][j][k], runs[1][j][k]
            assert np.array_equal(np.asarray(a), np.asarray(b)), (k, j)
    assert any(np.asarray(runs[0][3][k]).any() for k in D.KEYS)


@pytest.mark.parametrize("case", D.GRAD_CASES, ids=str)
def test_forward_half_is_the_inference_kernel(T, case):
    """Without a mask the features of the trainer's forward pass are the bits of BiLstmDecoderGPU.forward_torch on the same weights
    and frames: both run lstm_blocks.h's dot products, recurrent half and cell update, and the same head, term for term."""
    import torch
    from dss_amd.decoder import BiLstmDecoderGPU
    sd, x, y, _ = D.case_inputs(case, None)
    tr = T.DecoderTrainerGPU(sd, max_frames=case[2])
    for xs in (torch.from_numpy(x.astype(np.float32)), torch.from_numpy(x)):
        tr.trial(xs, y, mask=None, step=False)
        want = BiLstmDecoderGPU(1, case[2], state_dict=sd)(xs.cuda()[None])[0].cpu().numpy()
        assert np.array_equal(tr.features(), want)


def test_train_decoder_learns(T):
    from dss_amd.validation import decoder_validation
    sd, trials, corpus = D.learning_problem()
    L = D.LEARN
    args = (corpus["hga_activity"], corpus["lpc_coefficients"], corpus["trial_ids"])
    before = decoder_validation(sd, *args)
    best, hist = T.train_decoder(sd, corpus, corpus, epochs=L["epochs"], dropout=L["dropout"], lr=L["lr"], seed=L["seed"], shuffle=False)
    print(f"train_decoder: validation loss {before['loss']:.4f} -> " + ", ".join(f"{h['valid_loss']:.4f}" for h in hist) +
          f" (ratio {hist[-1]['valid_loss'] / before['loss']:.3f}, asserted below {D.LEARN_RATIO_GPU:.3f})")
    assert [h["update_steps"] for h in hist] == [6 * (e + 1) for e in range(L["epochs"])]
    assert D.LEARN_RATIO_GPU <= 0.75
    assert hist[-1]["valid_loss"] < D.LEARN_RATIO_GPU * before["loss"]
    assert all(np.isfinite(h["train_loss"]) for h in hist)
    kept = max(k for k, h in enumerate(hist) if h["best"])
    after = decoder_validation(best, *args)
    assert after["loss"] == hist[kept]["valid_loss"] == min(h["valid_loss"] for h in hist)
    # shuffled epochs from a seed are reproducible
    b1, h1 = T.train_decoder(sd, corpus, corpus, epochs=2, lr=L["lr"], seed=5)
    b2, h2 = T.train_decoder(sd, corpus, corpus, epochs=2, lr=L["lr"], seed=5)
    assert h1 == h2 and all(np.array_equal(b1[k].numpy(), b2[k].numpy()) for k in D.KEYS)
