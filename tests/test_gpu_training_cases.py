"""GPU tests of the two BPTT trainers (csrc/dec_train.hip, csrc/vad_train.hip, dss_amd/training.py) over the case table of
tests/training_cases.py: odd hidden and input sizes, the 8-frame tiles of the decoder's head and dmid kernels, trials and windows
beyond the 256-frame tile of the step kernels and beyond the loss loops' strides (512 / 640 frames), 1 to 32 outputs.

Per entry the gradients, the loss and the features / the carried state are held to float64 autograd with the helpers and bounds
of tests/test_gpu_decoder_training.py and tests/test_gpu_vad_training.py (``D.check_trial``, ``V.check_window``: GRAD_BOUND per
tensor, the loss bounds, lstm_reference.bound(scale), C_REL); tests/test_cpu_training_cases.py shows that the table fits that
bound's definition.  Both trainers' forward halves are the inference kernels bit for bit at every entry.  After update steps at
unaligned sizes the trainers are still the float64 model of the weights they read back, and what they publish is what loading
their ``state_dict()`` gives.  A handle that ran a long trial computes a short one like a fresh handle.  The detector's trial in
one call is its windows one by one at the window geometries no other test has, and the group forms equal their single trainers
at (7, 5) with trials on both sides of the tiles.  (The RMSprop formula at (7, 5, 9) and (33, 17, 17) runs in the two older files,
whose ``test_rmsprop_update_is_the_float64_formula`` takes ``TC.RMSPROP_CASES`` too.)"""
import numpy as np
import pytest

import lstm_reference as R
import decoder_training_reference as D
import vad_training_reference as V
import training_cases as TC

pytestmark = pytest.mark.gpu

LR = 1e-3


@pytest.fixture(scope="module")
def T():
    from dss_amd import training
    return training


def _x(x, f64=False):
    import torch
    return torch.from_numpy(x if f64 else x.astype(np.float32))


def _frame_types(e):
    return (False, True) if e.T <= TC.F64_FRAMES_UP_TO else (False,)


def _decoder_trial(H, C, n, seed, n_out):
    """A trial beside the table's: x (n, C) float64 holding float32 values, y (n, n_out) float32, mask (n, 2H) of 0 / 2."""
    x = R.frames("x2", 1, n, C, 8600 + seed)[0]
    rng = np.random.default_rng(9600 + seed)
    y = rng.standard_normal((n, n_out)).astype(np.float32)
    return x, y, (rng.random((n, 2 * H)) >= 0.5).astype(np.float32) * np.float32(2.0)


def _detector_trial(H, C, n, seed):
    """x (n, C) float64 holding float32 values, y (n,) uint8, mask (n, H) of 0 / 2."""
    x = R.frames("x2", 1, n, C, 8500 + seed)[0]
    rng = np.random.default_rng(9500 + seed)
    return x, rng.integers(0, 2, n).astype(np.uint8), (rng.random((n, H)) >= 0.5).astype(np.float32) * np.float32(2.0)


def _member(sd, k):
    """Weights of member k of a group: ``sd`` moved by a seeded perturbation, so that no two members are alike."""
    import torch
    if not k:
        return sd
    g = torch.Generator().manual_seed(4200 + k)
    return {n: v + 0.02 * torch.randn(v.shape, generator=g) for n, v in sd.items()}


def _same_dicts(a, b, keys, what):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


# ---- 1: gradients, loss, features / state against float64, per entry -----------------------------------------------------------

@pytest.mark.parametrize("e", TC.DECODER, ids=TC.ident)
def test_decoder_gradients_loss_and_features_against_float64(T, e):
    worst = np.zeros(3)
    tr = T.DecoderTrainerGPU(TC.decoder_inputs(e, None)[0], max_frames=e.T)
    assert tr.O == e.O
    for mask in e.masks:
        sd, x, y, m = TC.decoder_inputs(e, mask)
        for f64 in _frame_types(e):
            worst = np.maximum(worst, D.check_trial(tr, sd, x, y, m, e.scale, f64, f"decoder {TC.ident(e)} mask={mask} f64={f64}",
                                                    TC.decoder_truth(e, mask)))
    print(f"decoder {TC.ident(e)}: worst gradient {worst[0]:.3g} (bound {D.GRAD_BOUND:g}), loss {worst[1]:.3g}, features {worst[2]:.3g} "
          f"(bound {R.bound(e.scale):g})")


@pytest.mark.parametrize("e", TC.DETECTOR, ids=TC.ident)
def test_detector_gradients_loss_and_state_against_float64(T, e):
    worst = np.zeros(4)
    tr = T.VadTrainerGPU(TC.detector_inputs(e, None)[0], max_window=e.T)
    for mask in e.masks:
        sd, x, y, state, m = TC.detector_inputs(e, mask)
        assert np.any(state[0]) and np.any(state[1])       # from the case's carried state, not from zeros
        for f64 in _frame_types(e):
            worst = np.maximum(worst, V.check_window(tr, sd, x, y, state, m, e.scale, f64, f"detector {TC.ident(e)} mask={mask} f64={f64}",
                                                     TC.detector_truth(e, mask)))
    print(f"detector {TC.ident(e)}: worst gradient {worst[0]:.3g} (bound {V.GRAD_BOUND:g}), loss {worst[1]:.3g} (bound {2 * R.bound(e.scale):g}), "
          f"h {worst[2]:.3g} (bound {R.bound(e.scale):g}), c {worst[3]:.3g} (bound {R.C_REL:g})")


# ---- 2: the trainers' forward halves are the inference kernels --------------------------------------------------------------

@pytest.mark.parametrize("e", TC.DECODER, ids=TC.ident)
def test_decoder_forward_half_is_the_inference_kernel(T, e):
    """Without a mask the features of the trainer's forward pass are the bits of ``BiLstmDecoderGPU`` loaded from the same
    state_dict, with ``max_frames`` = T: at every output count and at the odd sizes."""
    from dss_amd.decoder import BiLstmDecoderGPU
    sd, x, y, _ = TC.decoder_inputs(e, None)
    tr = T.DecoderTrainerGPU(sd, max_frames=e.T)
    dec = BiLstmDecoderGPU(1, e.T, state_dict=sd)
    for xs in (_x(x), _x(x, True)):
        tr.trial(xs, y, mask=None, step=False)
        want = dec(xs.cuda()[None])[0].cpu().numpy()
        assert want.shape == (e.T, e.O) and np.isfinite(want).all() and want.any()
        assert np.array_equal(tr.features(), want)


@pytest.mark.parametrize("e", TC.DETECTOR, ids=TC.ident)
def test_detector_forward_half_is_the_inference_kernel(T, e):
    """Without a mask, two consecutive windows of a fresh trainer (the second from the state the first left) carry the bits of a
    fresh ``VadLstmGPU`` loaded from the same state_dict and stepped through the same frames twice: the state after each window,
    and the window's loss, which is what ``dss_vad_score_trials_dev`` makes of the detector's logits for those frames (the same
    term per frame, added in the same order, in float64)."""
    import torch
    from dss_amd import _lib
    from dss_amd.vad import VadLstmGPU
    sd, x, y, _, _ = TC.detector_inputs(e, None)
    L = _lib.require_gpu()
    tg = torch.from_numpy(np.ascontiguousarray(y, dtype=np.uint8)).cuda()
    length = np.array([e.T], np.int32)
    for f64 in _frame_types(e):
        tr, det, xs = T.VadTrainerGPU(sd, max_window=e.T), VadLstmGPU(1, state_dict=sd), _x(x, f64)
        for k in range(2):
            loss = tr.window(xs, y, mask=None, step=False)
            pred, logits = det.step_torch(xs.cuda()[None], want_logits=True)
            (h, c), (wh, wc) = tr.state(), det.state()
            assert np.array_equal(h, wh[:, 0]) and np.array_equal(c, wc[:, 0]), (f64, k)
            assert h.any() and c.any()
            want = torch.empty((1,), dtype=torch.float64, device="cuda")
            correct = torch.empty((1,), dtype=torch.int32, device="cuda")
            _lib.check(L.dss_vad_score_trials_dev(logits.data_ptr(), pred.data_ptr(), tg.data_ptr(), 1, length.ctypes.data, want.data_ptr(),
                                                  correct.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
            assert np.isfinite(loss) and loss == float(want.cpu()[0]), (f64, k, loss, float(want.cpu()[0]))


# ---- 3: after a step, still the float64 model of the read-back weights; publish ------------------------------------------------

@pytest.mark.parametrize("e", TC.DECODER_AFTER_STEPS, ids=TC.ident)
def test_decoder_after_steps_is_still_the_float64_model_of_its_weights(T, e):
    """Three update steps on fresh frames and masks.  Before each, ``state_dict()`` is read back; the step's gradients and features
    are held to autograd on THAT state_dict with the bounds of test 1: the packed weights the forward pass reads follow the master
    weights the update writes.  Then publish: bit for bit what loading ``state_dict()`` gives, and not the initial weights' output."""
    import torch
    from dss_amd.decoder import BiLstmDecoderGPU
    sd0 = TC.decoder_inputs(e, None)[0]
    tr = T.DecoderTrainerGPU(sd0, max_frames=e.T)
    for k in range(3):
        x, y, m = _decoder_trial(e.H, e.C, e.T, 10 * e.H + k, e.O)
        sd_k = tr.state_dict()
        if k:
            assert any(not np.array_equal(sd_k[n].numpy(), sd0[n].numpy()) for n in D.KEYS)
        loss = tr.trial(_x(x), y, mask=m, step=True, lr=LR)
        D.compare_trial(tr, loss, y, e.scale, f"decoder {TC.ident(e)} step {k}", D.autograd_trial(sd_k, x, y, m))
    dec = BiLstmDecoderGPU(1, e.T, state_dict=sd0)
    xs = _x(x).cuda()[None]
    before = dec(xs).clone()
    tr.publish(dec)
    got = dec(xs)
    assert torch.equal(got, BiLstmDecoderGPU(1, e.T, state_dict=tr.state_dict())(xs))
    assert not torch.equal(got, before)


@pytest.mark.parametrize("e", TC.DETECTOR_PUBLISH, ids=TC.ident)
def test_detector_publish_after_steps_is_loading_the_state_dict(T, e):
    import torch
    from dss_amd.vad import VadLstmGPU
    sd0 = TC.detector_inputs(e, None)[0]
    tr = T.VadTrainerGPU(sd0, max_window=e.T)
    for k in range(2):                                     # two stepped windows, the second from the state the first left
        x, y, m = _detector_trial(e.H, e.C, e.T, 10 * e.H + k)
        tr.window(_x(x), y, mask=m, step=True, lr=LR)
    det = VadLstmGPU(1, state_dict=sd0)
    xs = _x(x).cuda()[None]
    before = det.step_torch(xs, want_logits=True)[1].clone()
    det.reset()
    tr.publish(det)
    got = det.step_torch(xs, want_logits=True)[1]
    want = VadLstmGPU(1, state_dict=tr.state_dict()).step_torch(xs, want_logits=True)[1]
    assert torch.equal(got, want)
    assert not torch.equal(got, before)


# ---- 5: a reused handle is a fresh handle ---------------------------------------------------------------------------------------

def test_decoder_handle_reused_after_a_long_trial_is_a_fresh_handle(T):
    """513 frames, then 3 on the same handle: stash rows, ``lossf`` and the gate gradients beyond frame 3 are the long trial's, and
    nothing of them reaches the short one."""
    e, n = TC.DECODER_REUSE, TC.REUSE_FRAMES
    sd, x, y, m = TC.decoder_inputs(e, "random")
    xs, ys, ms = _decoder_trial(e.H, e.C, n, 77, e.O)
    tr = T.DecoderTrainerGPU(sd, max_frames=e.T)
    long_loss = tr.trial(_x(x), y, mask=m, step=False)
    assert np.isfinite(long_loss) and tr.features().shape == (e.T, e.O)
    got = (tr.trial(_x(xs), ys, mask=ms, step=False), tr.gradients(), tr.features())
    assert got[2].shape == (n, e.O) and any(got[1][k].any() for k in D.KEYS)
    for max_frames in (n, e.T):
        fresh = T.DecoderTrainerGPU(sd, max_frames=max_frames)
        assert fresh.trial(_x(xs), ys, mask=ms, step=False) == got[0], max_frames
        _same_dicts(fresh.gradients(), got[1], D.KEYS, f"gradients, max_frames {max_frames}")
        assert np.array_equal(fresh.features(), got[2]), max_frames


def test_detector_handle_reused_after_a_long_window_is_a_fresh_handle(T):
    e, n = TC.DETECTOR_REUSE, TC.REUSE_FRAMES
    sd, x, y, state, m = TC.detector_inputs(e, "random")
    xs, ys, ms = _detector_trial(e.H, e.C, n, 78)
    tr = T.VadTrainerGPU(sd, max_window=e.T)
    tr.set_state(*state)
    assert np.isfinite(tr.window(_x(x), y, mask=m, step=False))
    tr.set_state(*state)
    got = (tr.window(_x(xs), ys, mask=ms, step=False), tr.gradients(), tr.state())
    assert any(got[1][k].any() for k in V.KEYS)
    for max_window in (n, e.T):
        fresh = T.VadTrainerGPU(sd, max_window=max_window)
        fresh.set_state(*state)
        assert fresh.window(_x(xs), ys, mask=ms, step=False) == got[0], max_window
        _same_dicts(fresh.gradients(), got[1], V.KEYS, f"gradients, max_window {max_window}")
        h, c = fresh.state()
        assert np.array_equal(h, got[2][0]) and np.array_equal(c, got[2][1]), max_window


# ---- 6: the detector's trial and window geometry ----------------------------------------------------------------------------------

@pytest.mark.parametrize("H, C, n, window", TC.DETECTOR_TRIALS)
def test_detector_trial_in_one_call_is_its_windows_one_by_one(T, H, C, n, window):
    V.check_trial_is_its_windows(T, H, C, n, window=window)


# ---- 7: the group forms ---------------------------------------------------------------------------------------------------------

def test_decoder_group_step_at_odd_sizes_is_three_single_trainers(T):
    """Three members at (7, 5), 20 outputs, trials of 8, 9 and 257 frames, then the lengths rotated: every member is its single
    trainer bit for bit (loss, parameters, gradients, square averages, features), and the published copies agree."""
    import torch
    from dss_amd.decoder import BiLstmDecoderGPU
    H, C, O = 7, 5, 20
    frames, max_frames = TC.DECODER_GROUP_FRAMES, TC.DECODER_GROUP_MAX_FRAMES
    sds = [_member(R.decoder_state_dict(H, C, 1), m) for m in range(3)]
    steps = [[_decoder_trial(H, C, frames[(m + k) % 3], 100 + 10 * k + m, O) for m in range(3)] for k in range(2)]
    assert [len(s[0]) for s in steps[0]] == [8, 9, 257] and [len(s[0]) for s in steps[1]] == [9, 257, 8]
    g = T.DecoderGroupTrainerGPU(sds, max_frames=max_frames)
    singles = [T.DecoderTrainerGPU(sd, max_frames=max_frames) for sd in sds]
    for k, step in enumerate(steps):
        losses = g.step([_x(s[0]) for s in step], [s[1] for s in step], [s[2] for s in step], lr=LR).cpu().numpy()
        for m, (x, y, mask) in enumerate(step):
            want = singles[m].trial(_x(x), y, mask=mask, step=True, lr=LR)
            assert losses[m] == want, (k, m, losses[m], want)
            for name, a, b in (("parameters", g.state_dict(m), singles[m].state_dict()), ("gradients", g.gradients(m), singles[m].gradients()),
                               ("square averages", g.square_avg(m), singles[m].square_avg())):
                _same_dicts(a, b, D.KEYS, (k, m, name))
            assert np.array_equal(g.features(m), singles[m].features()), (k, m)
    xs = _x(steps[1][1][0]).cuda()[None]                   # the 257-frame trial
    outs = []
    for m in range(3):
        a, b = BiLstmDecoderGPU(1, max_frames, state_dict=sds[m]), BiLstmDecoderGPU(1, max_frames, state_dict=sds[m])
        before = a(xs).clone()
        g.publish(m, a)
        singles[m].publish(b)
        outs.append(a(xs).clone())
        assert torch.equal(outs[-1], b(xs)), (m, "published copies")
        assert not torch.equal(outs[-1], before), m
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])


def test_detector_group_trials_at_odd_sizes_are_three_single_trials(T):
    """One ``train_trials`` call of three members at (7, 5), trials of 16, 17 and 300 frames in windows of 8 (two windows, two and
    one frame, 37 and four frames) against three ``train_trial`` calls: losses, parameters, square averages, carried state (and
    the last window's gradients), bit for bit."""
    H, C = 7, 5
    W = TC.DETECTOR_GROUP_WINDOW
    sds = [_member(R.vad_state_dict(H, C, 1), m) for m in range(3)]
    trials = [_detector_trial(H, C, n, 200 + m) for m, n in enumerate(TC.DETECTOR_GROUP_FRAMES)]
    g = T.VadGroupTrainerGPU(sds, max_window=W)
    losses, counts = g.train_trials([_x(t[0]) for t in trials], [t[1] for t in trials], W, [t[2] for t in trials], lr=LR)
    losses = losses.cpu().numpy()
    assert list(counts) == [2, 3, 38] and losses.shape == (3, 38)
    for m, (x, y, mask) in enumerate(trials):
        tr = T.VadTrainerGPU(sds[m], max_window=W)
        want = tr.train_trial(_x(x), y, window=W, masks=mask, lr=LR)
        assert len(want) == counts[m] and np.array_equal(losses[m, :counts[m]], want), (m, losses[m], want)
        assert np.isnan(losses[m, counts[m]:]).all()
        for name, a, b in (("parameters", g.state_dict(m), tr.state_dict()), ("square averages", g.square_avg(m), tr.square_avg()),
                           ("gradients", g.gradients(m), tr.gradients())):
            _same_dicts(a, b, V.KEYS, (m, name))
        assert any(not np.array_equal(g.state_dict(m)[k].numpy(), np.asarray(sds[m][k])) for k in V.KEYS)
        (h, c), (wh, wc) = g.state(m), tr.state()
        assert np.array_equal(h, wh) and np.array_equal(c, wc) and h.any(), m
