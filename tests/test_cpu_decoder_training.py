"""CPU half of the checks of the decoder's training step (tests/decoder_training_reference.py is the reference of the GPU half):
the float64 reference is pinned to dss_amd.models.BidirectionalSpeechSynthesisModel, its written-out form to autograd, each
injected defect moves a gradient by more than 10 x the bound of the GPU test on that test's own inputs, the float64 run of the
learning problem learns, and bad sizes are refused without a device."""
import numpy as np
import pytest

import lstm_reference as R
import decoder_training_reference as D

SMALL = (D.GRAD_CASES[5], D.GRAD_CASES[2], D.GRAD_CASES[0], (16, 8, 9, 1))     # (6, 5, 7), (100, 64, 3), (100, 64, 1), the learning sizes


def _module64(sd, dropout=0.0):
    from dss_amd.models import BidirectionalSpeechSynthesisModel
    H4, C = sd["lstm.weight_ih_l0"].shape
    m = BidirectionalSpeechSynthesisModel(nb_layer=2, nb_hidden_units=H4 // 4, nb_electrodes=C, dropout=dropout).double()
    m.load_state_dict({k: v.double() for k, v in sd.items()})
    return m.train()


@pytest.mark.parametrize("case", SMALL + (D.GRAD_CASES[6],), ids=str)
def test_reference_is_the_models_class_in_float64(case):
    import torch
    sd, x, y, _ = D.case_inputs(case, None)
    m = _module64(sd)
    state = m.create_new_initial_state(batch_size=1)
    out, _ = m(torch.from_numpy(x)[None], (state[0].double(), state[1].double()))
    loss = torch.nn.MSELoss(reduction="mean")(out, torch.from_numpy(y.astype(np.float64))[None])
    loss.backward()
    want = {k: p.grad.numpy() for k, p in m.named_parameters()}
    got_loss, got, feat = D.autograd_trial(sd, x, y, None)
    assert set(want) == set(D.KEYS)
    assert abs(got_loss - float(loss.detach())) <= 1e-12
    for k in D.KEYS:
        assert np.abs(got[k] - want[k]).max() <= 1e-12, k
    assert np.abs(feat - out.detach().numpy()[0]).max() <= 1e-12


def test_keys_are_the_decoders():
    from dss_amd import decoder
    assert D.KEYS == decoder._KEYS


@pytest.mark.parametrize("mask", (None, "random", "zero_row"))
@pytest.mark.parametrize("case", SMALL + (D.GRAD_CASES[8],), ids=str)
def test_written_out_trial_is_autograd(case, mask):
    sd, x, y, m = D.case_inputs(case, mask)
    l0, g0, f0 = D.autograd_trial(sd, x, y, m)
    l1, g1, f1 = D.manual_trial(sd, x, y, m)
    assert abs(l0 - l1) <= 1e-12
    for k in D.KEYS:
        assert np.abs(g0[k] - g1[k]).max() <= 1e-12 * max(1.0, np.abs(g0[k]).max()), k
    assert np.abs(f0 - f1).max() <= 1e-12


def test_reference_loop_is_the_scripts_loop():
    """train_bidirectional_model.py:134-152 on the models class (float64, dropout 0), two trials: the same final parameters."""
    import torch
    sd = R.decoder_state_dict(16, 8, 1)
    rng = np.random.default_rng(5)
    trials = [(rng.standard_normal((n, 8)), rng.standard_normal((n, 20))) for n in (23, 17)]
    m = _module64(sd)
    optim = torch.optim.RMSprop(m.parameters(), lr=0.0001)
    cfunc = torch.nn.MSELoss(reduction="mean")
    for x, y in trials:
        x_train, y_train = torch.from_numpy(x)[None], torch.from_numpy(y)[None]
        init_state = m.create_new_initial_state(batch_size=1)
        init_state = (init_state[0].double(), init_state[1].double())
        for param in m.parameters():
            param.grad = None
        pred, _ = m(x_train, state=init_state)
        loss = cfunc(pred, y_train)
        loss.backward()
        optim.step()
    got, losses = D.reference_loop(sd, trials, masks=None, lr=0.0001)
    assert len(losses) == 2
    for k, p in m.state_dict().items():
        assert np.abs(got[k].numpy() - p.numpy()).max() <= 1e-12, k


@pytest.fixture(scope="module")
def truths():
    out = {}
    for case in D.GRAD_CASES:
        inputs = D.case_inputs(case, "random")
        out[case] = (inputs, D.manual_trial(*inputs)[1])
    return out


@pytest.mark.parametrize("defect", D.DEFECTS)
def test_each_defect_exceeds_ten_bounds(defect, truths):
    """Power: on the gradient cases' own inputs every defect moves at least one tensor by more than 10 x GRAD_BOUND on at least one
    case -- a kernel with that defect cannot pass the GPU test."""
    worst = 0.0
    for case, (inputs, want) in truths.items():
        got = D.manual_trial(*inputs, defect=defect)[1]
        worst = max(worst, max(D.rel_errors(got, want).values()))
        if worst > 10 * D.GRAD_BOUND:
            break
    print(defect, worst)
    assert worst > 10 * D.GRAD_BOUND


def test_float64_run_of_the_learning_problem_learns():
    sd, trials, _ = D.learning_problem()
    L = D.LEARN
    before = D.validation_loss64(sd, trials)
    got, losses = D.reference_loop(sd, trials, masks=D.learning_masks(trials), lr=L["lr"], epochs=L["epochs"])
    after = D.validation_loss64({k: v.numpy() for k, v in got.items()}, trials)
    print(f"float64 reference: validation loss {before:.4f} -> {after:.4f} (ratio {after / before:.3f}), {len(losses)} update steps")
    assert len(losses) == 6 * L["epochs"]
    assert D.LEARN_RATIO_CPU <= 0.5
    assert after < D.LEARN_RATIO_CPU * before


@pytest.mark.parametrize("args, word", [((64, 100, 20, 2048, 0), "trial of 0"), ((64, 100, 20, 2048, 2049), "trial of 2049"),
                                        ((64, 129, 20, 2048, 1), "129 hidden"), ((257, 100, 20, 2048, 1), "257 inputs"),
                                        ((64, 100, 33, 2048, 1), "33 outputs"), ((64, 100, 20, 0, 1), "max_frames 0"),
                                        ((64, 100, 20, 5000, 1), "max_frames 5000"), ((0, 100, 20, 2048, 1), "0 inputs")])
def test_bad_sizes_are_refused_without_a_device(args, word):
    from dss_amd import _lib
    L = _lib.load()
    assert L.dss_dec_trainer_check(*args) == -1           # DSS_EINVAL
    assert word in L.dss_last_error().decode()
    assert L.dss_dec_trainer_check(64, 100, 20, 2048, 1500) == 0 and L.dss_dec_trainer_check(256, 128, 32, 4096, 4096) == 0


def test_python_layer_refuses_bad_models_and_sizes():
    import torch
    from dss_amd import _lib
    from dss_amd import training
    from dss_amd.training import DecoderTrainerGPU, decoder_dropout_mask
    sd = R.decoder_state_dict(6, 5, 1)
    with pytest.raises(_lib.DssError, match="max_frames 0"):
        DecoderTrainerGPU(sd, max_frames=0)
    with pytest.raises(ValueError, match="architecture"):
        DecoderTrainerGPU({k: v for k, v in sd.items() if k != "regressor.bias"})
    with pytest.raises(ValueError, match="architecture"):
        DecoderTrainerGPU(R.vad_state_dict(6, 5, 1))
    # the shape checks run before anything touches a device
    tr = DecoderTrainerGPU.__new__(DecoderTrainerGPU)
    tr.C, tr.H, tr.O = 5, 6, 20
    with pytest.raises(ValueError, match=r"mask must be \(7, 12\)"):
        tr._mask(np.zeros((7, 6), np.float32), 7)
    with pytest.raises(ValueError, match=r"targets must be \(7, 20\)"):
        tr._targets(np.zeros((7, 4), np.float32), 7)
    with pytest.raises(ValueError, match=r"frames must be \(T, 5\)"):
        tr._frames(np.zeros((7, 6), np.float32))
    m = decoder_dropout_mask(40, 6, 0.5, torch.Generator().manual_seed(1)).numpy()
    assert m.shape == (40, 12) and set(np.unique(m)) == {0.0, 2.0} and decoder_dropout_mask(40, 6, 0.0, None) is None
    with pytest.raises(ValueError):
        decoder_dropout_mask(40, 6, 1.0, None)
    assert _lib.load().dss_dec_trainer_param_count(5, 6, 20) == sum(int(np.prod(v.shape)) for v in sd.values())
    assert {"DecoderTrainerGPU", "train_decoder", "decoder_dropout_mask"} <= set(training.__all__)
