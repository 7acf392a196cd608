"""The detector's training step on the GPU (csrc/vad_train.hip, dss_amd/training.py) against the float64 references of
tests/vad_training_reference.py: gradients, loss and carried state per window; the RMSprop update against the float64 formula on
the kernel's own read-back values; a trial in one call against its windows one by one, bit for bit; publish; learning.

Bounds: gradients V.GRAD_BOUND per tensor (max|g - g64| / max|g64|; 4 x torch float32 CPU autograd's own error, see the helper);
loss 2 x lstm_reference.bound(scale) (the cross-entropy's gradient in the two logits has L1 norm <= 2, the logits hold `bound`);
new h within bound(scale), new c within C_REL like the precision tests."""
import numpy as np
import pytest

import lstm_reference as R
import vad_training_reference as V
import training_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    from dss_amd import training
    return training


def _check_window(*args, **kw):
    """The checker lives in the helper module (tests/test_gpu_training_cases.py runs it too); the worst gradient error."""
    return V.check_window(*args, **kw)[0]


@pytest.mark.parametrize("case", V.GRAD_CASES, ids=str)
def test_gradients_loss_and_state_against_float64(T, case):
    worst = 0.0
    tr = None
    for j, mask in enumerate((None, "random")):
        sd, x, y, state, m = V.case_inputs(case, mask)
        tr = tr or T.VadTrainerGPU(sd, max_window=50)
        for f64 in (False, True):
            worst = max(worst, _check_window(tr, sd, x, y, state, m, case[3], f64, f"{case} mask={mask} f64={f64}"))
    print(f"{case}: worst gradient error {worst:.3g} (bound {V.GRAD_BOUND:g})")


@pytest.mark.parametrize("mask, targets", [("zero_row", "random"), ("random", "one_class")])
def test_zero_mask_row_and_one_class_window(T, mask, targets):
    case = V.GRAD_CASES[0]
    sd, x, y, state, m = V.case_inputs(case, mask, targets)
    _check_window(T.VadTrainerGPU(sd, max_window=50), sd, x, y, state, m, 1, False, f"{case} mask={mask} targets={targets}")


def test_window_sizes_are_checked(T):
    from dss_amd import _lib
    sd, x, y, state, m = V.case_inputs(V.GRAD_CASES[5], None)
    tr = T.VadTrainerGPU(sd, max_window=4)
    with pytest.raises(_lib.DssError, match="window of 7"):
        tr.window(x, y)
    with pytest.raises(_lib.DssError, match="windows of 5"):
        tr.train_trial(x, y, window=5)


def _ulp32(v):
    v = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


@pytest.mark.parametrize("case", (V.GRAD_CASES[0], V.GRAD_CASES[5]) + TC.RMSPROP_CASES, ids=str)
def test_rmsprop_update_is_the_float64_formula(T, case):
    """Two consecutive steps (the first from sq = 0): p', sq' against the float64 formula on the read-back float32 p, sq and the
    kernel's own g; bias_ih / bias_hh: equal g, separate updates; step=False leaves p and sq bit-identical; publish: b0 = b_ih + b_hh."""
    from dss_amd.vad import VadLstmGPU
    sd, x, y, state, m = V.case_inputs(case, "random")
    tr = T.VadTrainerGPU(sd, max_window=50)
    tr.set_state(*state)
    lr, alpha, eps = 1e-3, 0.99, 1e-8
    u = 2.0 ** -24
    for step in range(2):
        p0, s0 = tr.state_dict(), tr.square_avg()
        tr.window(x, y, mask=m, step=False)
        assert all(np.array_equal(p0[k].numpy(), tr.state_dict()[k].numpy()) for k in V.KEYS)
        assert all(np.array_equal(s0[k], tr.square_avg()[k]) for k in V.KEYS)
        tr.set_state(*state)
        tr.window(x, y, mask=m, step=True, lr=lr, alpha=alpha, eps=eps)
        g, p1, s1 = tr.gradients(), tr.state_dict(), tr.square_avg()
        tr.set_state(*state)
        if step == 0:
            assert all(not s0[k].any() for k in V.KEYS)
        for k in V.KEYS:
            pw, sw = V.rmsprop64(p0[k].numpy(), s0[k], g[k], lr, alpha, eps)
            assert (np.abs(s1[k] - sw) <= 4 * u * sw).all(), (step, k)
            dp = np.abs(pw - p0[k].numpy().astype(np.float64))
            assert (np.abs(p1[k].numpy() - pw) <= _ulp32(pw) + 4 * u * dp).all(), (step, k)
            assert np.abs(dp).max() > 0
        for layer in (0, 1):
            assert np.array_equal(g[f"lstm.bias_ih_l{layer}"], g[f"lstm.bias_hh_l{layer}"])
        if step == 1:          # the two biases started apart, so equal g moved them by the same formula from different p
            assert not np.array_equal(p1["lstm.bias_ih_l0"].numpy(), p1["lstm.bias_hh_l0"].numpy())
    # the packed copies follow the master parameters: a published handle computes what a handle loaded from state_dict() computes
    det = VadLstmGPU(1, state_dict=sd)
    tr.publish(det)
    import torch
    xs = torch.from_numpy(x.astype(np.float32)).cuda()[None]
    _, got = det.step_torch(xs, want_logits=True)
    _, want = VadLstmGPU(1, state_dict=tr.state_dict()).step_torch(xs, want_logits=True)
    assert torch.equal(got, want)


TRIALS = [(16, 8, 120), (16, 8, 101), (150, 64, 120), (150, 64, 101)]


@pytest.mark.parametrize("H, C, n", TRIALS)
def test_trial_in_one_call_is_its_windows_one_by_one(T, H, C, n):
    V.check_trial_is_its_windows(T, H, C, n, window=50)   # (tests/test_gpu_training_cases.py runs it at other windows)


def test_publish_then_validation_is_validation_of_the_state_dict(T):
    from dss_amd.vad import VadLstmGPU
    from dss_amd.validation import vad_validation
    sd, trials, corpus = V.learning_problem()
    tr = T.VadTrainerGPU(sd, max_window=50)
    for k, (x, y) in enumerate(trials[:3]):
        tr.train_trial(x, y, window=50, masks=V.learning_masks(trials)[0][k], lr=1e-3)
    det = VadLstmGPU(1, state_dict=sd)
    import torch
    det.step_torch(torch.from_numpy(trials[0][0][:4].astype(np.float32)).cuda()[None])       # a streaming state that is not zero
    h0, c0 = det.state()
    tr.publish(det)
    a = vad_validation(det, corpus["hga_activity"], corpus["vad_labels"], corpus["trial_ids"])
    b = vad_validation(tr.state_dict(), corpus["hga_activity"], corpus["vad_labels"], corpus["trial_ids"])
    before = vad_validation(sd, corpus["hga_activity"], corpus["vad_labels"], corpus["trial_ids"])
    assert np.array_equal(a["pred"], b["pred"]) and np.array_equal(a["prob"], b["prob"])
    assert np.array_equal(a["per_trial_loss"], b["per_trial_loss"])
    assert not np.array_equal(a["prob"], before["prob"])
    h1, c1 = det.state()
    assert np.array_equal(h0, h1) and np.array_equal(c0, c1) and h0.any()


def test_train_vad_learns(T):
    from dss_amd.validation import vad_validation
    sd, trials, corpus = V.learning_problem()
    L = V.LEARN
    before = vad_validation(sd, corpus["hga_activity"], corpus["vad_labels"], corpus["trial_ids"])
    best, hist = T.train_vad(sd, corpus, corpus, epochs=L["epochs"], window=L["window"], dropout=L["dropout"], lr=L["lr"],
                             seed=L["seed"], shuffle=False)
    print(f"train_vad: validation loss {before['loss']:.4f} -> " + ", ".join(f"{h['valid_loss']:.4f}" for h in hist) +
          f"; accuracy {before['accuracy']:.3f} -> " + ", ".join(f"{h['accuracy']:.3f}" for h in hist))
    assert [h["update_steps"] for h in hist] == [17, 34, 51]
    assert hist[-1]["valid_loss"] < 0.5 * before["loss"]
    assert hist[-1]["accuracy"] > before["accuracy"]
    kept = max(k for k, h in enumerate(hist) if h["best"])
    after = vad_validation(best, corpus["hga_activity"], corpus["vad_labels"], corpus["trial_ids"])
    assert after["accuracy"] == hist[kept]["accuracy"] == max(h["accuracy"] for h in hist)
    # shuffled epochs from a seed are reproducible
    b1, h1 = T.train_vad(sd, corpus, corpus, epochs=1, lr=L["lr"], seed=5)
    b2, h2 = T.train_vad(sd, corpus, corpus, epochs=1, lr=L["lr"], seed=5)
    assert h1 == h2 and all(np.array_equal(b1[k].numpy(), b2[k].numpy()) for k in V.KEYS)
