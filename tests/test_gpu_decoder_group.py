"""Several decoders trained at once on the GPU (``DecoderGroupTrainerGPU`` / ``train_decoders``, the group kernels of
csrc/dec_train.hip) against the single trainer (``DecoderTrainerGPU``), which tests/test_gpu_decoder_training.py pins to float64
autograd.  For every model, after every sequence of group steps, the loss, the features, the gradients, the square averages, the
parameters and the published packed copies are BIT-IDENTICAL (``np.array_equal`` on the raw float32 arrays, no tolerance) to a
single trainer loaded with the same weights and given that model's trials in the same order -- whatever M is, wherever the model
sits and whatever the other models do in the same step.  One test holds the group path to ``D.autograd_trial`` directly."""
import numpy as np
import pytest

import lstm_reference as R
import decoder_training_reference as D

pytestmark = pytest.mark.gpu

O = 20


@pytest.fixture(scope="module")
def T():
    from dss_amd import training
    return training


def _member_sd(H, C, k, scale=1):
    """Weights of member k: the precision tests' decoder, moved by a seeded perturbation so that no two members are alike."""
    import torch
    sd = R.decoder_state_dict(H, C, scale)
    if k:
        g = torch.Generator().manual_seed(4000 + k)
        sd = {n: v + 0.02 * torch.randn(v.shape, generator=g) for n, v in sd.items()}
    return sd


def _trial(H, C, n, seed, mask="random", n_out=O):
    """x (n, C) float64 holding float32 values, y (n, n_out) float32, mask (n, 2H) multipliers of 0 / 2 or None."""
    x = R.frames("x2", 1, n, C, 8800 + seed)[0]
    rng = np.random.default_rng(9900 + seed)
    y = rng.standard_normal((n, n_out)).astype(np.float32)
    m = None
    if mask is not None:
        m = (rng.random((n, 2 * H)) >= 0.5).astype(np.float32) * np.float32(2.0)
        if mask == "zero_row":
            m[n // 2] = 0.0
    return x, y, m


def _x(x, f64=False):
    import torch
    return None if x is None else torch.from_numpy(x if f64 else x.astype(np.float32))


def _assert_member_is(g, m, tr, what=""):
    """Parameters, gradients, square averages and the features of the last trial, bit for bit."""
    for name, a, b in (("parameters", g.state_dict(m), tr.state_dict()), ("gradients", g.gradients(m), tr.gradients()),
                       ("square averages", g.square_avg(m), tr.square_avg())):
        for k in D.KEYS:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, m, name, k)
    assert np.array_equal(g.features(m), tr.features()), (what, m, "features")


def _assert_published_is(g, m, tr, sd0, x, max_frames):
    """The packed copies: published into inference handles, both compute the same bits."""
    import torch
    from dss_amd.decoder import BiLstmDecoderGPU
    a, b = BiLstmDecoderGPU(1, max_frames, state_dict=sd0), BiLstmDecoderGPU(1, max_frames, state_dict=sd0)
    g.publish(m, a)
    tr.publish(b)
    xs = torch.from_numpy(x.astype(np.float32)).cuda()[None]
    assert torch.equal(a(xs), b(xs)), (m, "published copies")


def _run_both(T, sds, steps, max_frames, f64=False, lr=1e-3, apply=None):
    """steps[k][m] = (x, y, mask) or None.  Runs the group and M single trainers; compares the losses of every step and all
    read-backs after every step.  Returns (group, single trainers)."""
    M = len(sds)
    g = T.DecoderGroupTrainerGPU(sds, max_frames=max_frames)
    singles = [T.DecoderTrainerGPU(sd, max_frames=max_frames) for sd in sds]
    lrs = lr if isinstance(lr, (list, tuple)) else [lr] * M
    for k, step in enumerate(steps):
        ap = True if apply is None else apply[k]
        losses = g.step([None if s is None else _x(s[0], f64) for s in step], [None if s is None else s[1] for s in step],
                        [None if s is None else s[2] for s in step], apply=ap, lr=lrs).cpu().numpy()
        for m, s in enumerate(step):
            if s is None:
                assert np.isnan(losses[m])
                continue
            want = singles[m].trial(_x(s[0], f64), s[1], mask=s[2], step=ap, lr=lrs[m])
            assert losses[m] == want, (k, m, losses[m], want)
            _assert_member_is(g, m, singles[m], f"step {k}")
    return g, singles


# ---- 1, 7: the mixed step --------------------------------------------------------------------------------------------------------

MIX_LENGTHS = (1, 5, 37)          # one frame: weight_hh gradients exactly zero; 5: no multiple of DEC_TP = 4 or of the 8-frame tiles; 37: ragged
MIX_MASKS = (None, "random", "zero_row")
MIX_SCALES = (1, 4, 1)


@pytest.fixture(scope="module")
def mixed():
    sds = [R.decoder_state_dict(100, 64, s) for s in MIX_SCALES]
    steps = [[_trial(100, 64, MIX_LENGTHS[(m + k) % 3], 10 * k + m, MIX_MASKS[m]) for m in range(3)] for k in range(3)]
    return sds, steps


@pytest.mark.parametrize("f64", (False, True), ids=("float32 frames", "float64 frames"))
def test_mixed_step_is_three_single_trainers(T, mixed, f64):
    sds, steps = mixed
    assert sorted(len(s[0]) for s in steps[0]) == [1, 5, 37] and {len(steps[k][0][0]) for k in range(3)} == {1, 5, 37}
    g, singles = _run_both(T, sds, steps, 37, f64=f64, apply=(False, True, True))
    one = [k for k in range(3) if len(steps[2][k][0]) == 1][0]
    assert not g.gradients(one)["lstm.weight_hh_l0"].any() and not g.gradients(one)["lstm.weight_hh_l1_reverse"].any()
    for m in range(3):
        _assert_published_is(g, m, singles[m], sds[m], steps[2][2][0], 37)


def test_group_step_against_float64_autograd(T, mixed):
    """Member 1 (weights x 4, five frames, a random mask) of the first mixed step against D.autograd_trial: gradients within
    D.GRAD_BOUND, features within R.bound(4) -- the group path held to the float64 reference directly."""
    sds, steps = mixed
    g = T.DecoderGroupTrainerGPU(sds, max_frames=37)
    g.step([_x(s[0]) for s in steps[0]], [s[1] for s in steps[0]], [s[2] for s in steps[0]], apply=False)
    x, y, m = steps[0][1]
    assert len(x) == 5 and m is not None
    _, want_g, want_f = D.autograd_trial(sds[1], x, y, m)
    err = D.rel_errors(g.gradients(1), want_g)
    ef = float(np.abs(g.features(1) - want_f).max())
    print(f"group member 1: gradient {max(err.values()):.3g} ({max(err, key=err.get)}; bound {D.GRAD_BOUND:g}), features {ef:.3g} "
          f"(bound {R.bound(MIX_SCALES[1]):g})")
    for k in D.KEYS:
        assert err[k] <= D.GRAD_BOUND, (k, err[k])
    assert ef <= R.bound(MIX_SCALES[1])


# ---- 2: capacity corners -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H, C, n, M", [(128, 256, 9, 2), (6, 5, 7, 4)])
def test_capacity_corners(T, H, C, n, M):
    sds = [_member_sd(H, C, m) for m in range(M)]
    steps = [[_trial(H, C, n, 100 * k + m + H) for m in range(M)] for k in range(2)]
    g, singles = _run_both(T, sds, steps, n)
    _assert_published_is(g, M - 1, singles[M - 1], sds[M - 1], steps[0][0][0], n)


# ---- 3: sitting out ----------------------------------------------------------------------------------------------------------------

def test_a_model_that_sits_out_is_left_alone(T):
    import torch
    H, C = 16, 8
    sds = [_member_sd(H, C, m) for m in range(3)]
    first = [_trial(H, C, n, 300 + m) for m, n in enumerate((9, 12, 5))]
    second = [_trial(H, C, 11, 310), None, _trial(H, C, 4, 312)]
    g, singles = _run_both(T, sds, [first], 12)
    before = (g.state_dict(1), g.gradients(1), g.square_avg(1), g.features(1))
    from dss_amd.decoder import BiLstmDecoderGPU
    dec = BiLstmDecoderGPU(1, 12, state_dict=sds[1])
    xs = torch.from_numpy(first[1][0].astype(np.float32)).cuda()[None]
    g.publish(1, dec)
    packed_before = dec(xs).clone()
    losses = torch.full((3,), 12345.0, dtype=torch.float64, device="cuda")
    out = g.step([_x(s[0]) if s else None for s in second], [s[1] if s else None for s in second], [s[2] if s else None for s in second],
                 lr=1e-3, losses=losses)
    assert out is losses
    got = losses.cpu().numpy()
    assert got[1] == 12345.0                               # the sentinel: the loss slot of the model that sat out is not written
    after = (g.state_dict(1), g.gradients(1), g.square_avg(1), g.features(1))
    for a, b in zip(before[:3], after[:3]):
        assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in D.KEYS)
    assert np.array_equal(before[3], after[3]) and after[3].shape == (12, O)
    g.publish(1, dec)
    assert torch.equal(dec(xs), packed_before)
    for m in (0, 2):
        assert got[m] == singles[m].trial(_x(second[m][0]), second[m][1], mask=second[m][2], step=True, lr=1e-3)
        _assert_member_is(g, m, singles[m], "second step")
    _assert_member_is(g, 1, singles[1], "sat out")


# ---- 4: position and width ---------------------------------------------------------------------------------------------------------

def _other_length(j, k, taken):
    """1 .. 11 frames, varying with the member and the step, never the length of the trial under test."""
    n = 1 + (5 * j + 3 * k + 1) % 11
    return n if n != taken else n % 11 + 1


def test_position_in_the_group_and_its_width_change_no_bit(T):
    H, C = 16, 8
    sd = _member_sd(H, C, 99)
    mine = [_trial(H, C, n, 400 + k) for k, n in enumerate((12, 3, 8))]
    single = T.DecoderTrainerGPU(sd, max_frames=12)
    want = []
    for x, y, m in mine:
        loss = single.trial(_x(x), y, mask=m, step=True, lr=1e-3)
        want.append((loss, single.state_dict(), single.gradients(), single.square_avg(), single.features()))
    for M, pos in ((1, 0), (5, 4), (64, 63)):
        sds = [_member_sd(H, C, m) for m in range(M)]
        sds[pos] = sd
        g = T.DecoderGroupTrainerGPU(sds, max_frames=12)
        assert len(g) == M
        for k, (x, y, m) in enumerate(mine):
            others = {j: _trial(H, C, _other_length(j, k, len(x)), 1000 * k + j, ("random", None)[j % 2]) for j in range(M) if j != pos}
            assert all(len(o[0]) <= 12 and len(o[0]) != len(x) for o in others.values())
            step = [(x, y, m) if j == pos else others[j] for j in range(M)]
            losses = g.step([_x(s[0]) for s in step], [s[1] for s in step], [s[2] for s in step], lr=1e-3).cpu().numpy()
            loss, p, gr, sq, f = want[k]
            assert losses[pos] == loss, (M, k)
            for name, a, b in (("parameters", g.state_dict(pos), p), ("gradients", g.gradients(pos), gr), ("square averages", g.square_avg(pos), sq)):
                assert all(np.array_equal(np.asarray(a[q]), np.asarray(b[q])) for q in D.KEYS), (M, k, name)
            assert np.array_equal(g.features(pos), f), (M, k)
            if M == 64 and k == 0:                         # every other member of the widest group, on its one trial
                for j, (ox, oy, om) in others.items():
                    tr = T.DecoderTrainerGPU(sds[j], max_frames=12)
                    assert losses[j] == tr.trial(_x(ox), oy, mask=om, step=True, lr=1e-3), j
                    _assert_member_is(g, j, tr, "M = 64")


# ---- 5: a learning rate per model --------------------------------------------------------------------------------------------------

def test_learning_rate_per_model(T):
    H, C = 16, 8
    sds = [_member_sd(H, C, 7)] * 3                        # the same weights and trials: only the learning rate tells the models apart
    steps = [[_trial(H, C, 10, 500 + k)] * 3 for k in range(2)]
    g, _ = _run_both(T, sds, steps, 10, lr=[1e-4, 3e-3, 1e-2])
    a, b, c = (g.state_dict(m)["lstm.weight_ih_l0"].numpy() for m in range(3))
    assert not np.array_equal(a, b) and not np.array_equal(b, c)


# ---- 6: back to back: the table ring -----------------------------------------------------------------------------------------------

def test_steps_enqueued_back_to_back(T):
    """Four steps with four length tables, enqueued with nothing in between that waits for the device (frames, targets and masks
    are on the device before the first): every step reads its own table."""
    import torch
    H, C, M = 16, 8, 3
    tables = ((12, 3, 7), (2, 11, 0), (5, 5, 9), (0, 8, 1))
    sds = [_member_sd(H, C, m) for m in range(M)]
    steps = [[_trial(H, C, n, 600 + 10 * k + m) if n else None for m, n in enumerate(tab)] for k, tab in enumerate(tables)]
    dev = [[None if s is None else tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in s) for s in step]
           for step in steps]
    g = T.DecoderGroupTrainerGPU(sds, max_frames=12)
    torch.cuda.synchronize()
    losses = [g.step([s and s[0] for s in step], [s and s[1] for s in step], [s and s[2] for s in step], lr=1e-3) for step in dev]
    losses = torch.stack(losses).cpu().numpy()
    for m in range(M):
        tr = T.DecoderTrainerGPU(sds[m], max_frames=12)
        for k, step in enumerate(steps):
            if step[m] is None:
                assert np.isnan(losses[k, m])
            else:
                assert losses[k, m] == tr.trial(_x(step[m][0]), step[m][1], mask=step[m][2], step=True, lr=1e-3), (k, m)
        _assert_member_is(g, m, tr, "after four steps")


# ---- 8: publish --------------------------------------------------------------------------------------------------------------------

def test_publish_of_a_member_is_loading_its_state_dict(T):
    import torch
    from dss_amd.decoder import BiLstmDecoderGPU
    case = D.GRAD_CASES[6]
    sd, x, y, m = D.case_inputs(case, "random")
    sds = [_member_sd(100, 64, 1), sd]
    g = T.DecoderGroupTrainerGPU(sds, max_frames=64)
    other = _trial(100, 64, 21, 800)
    for _ in range(2):
        g.step([_x(other[0]), _x(x)], [other[1], y], [other[2], m], lr=1e-3)
    dec = BiLstmDecoderGPU(1, 64, state_dict=sd)
    xs = torch.from_numpy(x.astype(np.float32)).cuda()[None]
    before = dec(xs).clone()
    g.publish(1, dec)
    got = dec(xs)
    assert torch.equal(got, BiLstmDecoderGPU(1, 64, state_dict=g.state_dict(1))(xs))
    assert not torch.equal(got, before)
    assert not torch.equal(got, BiLstmDecoderGPU(1, 64, state_dict=g.state_dict(0))(xs))
    with pytest.raises(Exception, match="inputs"):
        g.publish(1, BiLstmDecoderGPU(1, 64, state_dict=R.decoder_state_dict(16, 8, 1)))
    with pytest.raises(IndexError):
        g.publish(2, dec)


# ---- 9: the epoch loops ------------------------------------------------------------------------------------------------------------

def _head(corpus, trials, n):
    rows = sum(len(y) for _, y in trials[:n])
    return {k: v[:rows] for k, v in corpus.items()}


@pytest.mark.parametrize("shuffle, epochs", [(False, D.LEARN["epochs"]), (True, 2)])
def test_train_decoders_is_train_decoder_per_model(T, shuffle, epochs):
    from dss_amd.validation import decoder_validation
    sd, trials, corpus = D.learning_problem()
    L = D.LEARN
    seeds = (11, 12, 13)
    corpora = [_head(corpus, trials, n) for n in (6, 5, 4)]    # models 1 and 2 sit out the last steps of every epoch
    got = T.train_decoders([sd] * 3, corpora, [corpus] * 3, epochs=epochs, dropout=L["dropout"], lr=L["lr"], seeds=seeds, shuffle=shuffle)
    assert len(got) == 3
    for m in range(3):
        best, hist = T.train_decoder(sd, corpora[m], corpus, epochs=epochs, dropout=L["dropout"], lr=L["lr"], seed=seeds[m], shuffle=shuffle)
        assert got[m][1] == hist, (m, got[m][1], hist)
        assert [h["update_steps"] for h in hist] == [(6 - m) * (e + 1) for e in range(epochs)]
        assert all(np.array_equal(got[m][0][k].numpy(), best[k].numpy()) for k in D.KEYS), m
    if not shuffle:                                        # model 0 is the run of the single trainer's learning test
        before = decoder_validation(sd, corpus["hga_activity"], corpus["lpc_coefficients"], corpus["trial_ids"])
        ratio = got[0][1][-1]["valid_loss"] / before["loss"]
        print(f"train_decoders, model 0: validation loss ratio {ratio:.3f} (asserted below {D.LEARN_RATIO_GPU:.3f})")
        assert ratio < D.LEARN_RATIO_GPU


# ---- 10: refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals(T):
    from dss_amd import _lib
    H, C = 6, 5
    sds = [_member_sd(H, C, m) for m in range(2)]
    g = T.DecoderGroupTrainerGPU(sds, max_frames=8)
    x, y, m = _trial(H, C, 7, 900)
    long = _trial(H, C, 9, 901)
    before = g.state_dict(0)
    with pytest.raises(ValueError, match="trial of 9 frames"):
        g.step([_x(x), _x(long[0])], [y, long[1]])
    with pytest.raises(ValueError, match="mask must be"):
        g.step([_x(x), _x(x)], [y, y], [m, np.zeros((7, 6), np.float32)])
    with pytest.raises(ValueError, match="every model sits out"):
        g.step([None, None], [None, None])
    with pytest.raises(ValueError, match="3 entries for 2 models"):
        g.step([_x(x)] * 3, [y] * 3)
    with pytest.raises(ValueError, match="1 entries for 2 models"):
        g.step([_x(x)] * 2, [y] * 2, lr=[1e-3])
    with pytest.raises(TypeError, match="one dtype"):
        g.step([_x(x), _x(x, True)], [y, y])
    assert all(np.array_equal(before[k].numpy(), g.state_dict(0)[k].numpy()) for k in D.KEYS)      # nothing was launched
    L = _lib.load()
    for n in (0, 65):
        assert L.dss_dec_group_check(n, C, H, O, 8) == -1 and f"{n} models" in L.dss_last_error().decode()
    # the C ABI's own refusals, behind the class's: T beyond max_frames, and a step of zeros
    import ctypes as Ct
    import torch
    tab = (T._GroupTrial * 2)()
    losses = torch.zeros(2, dtype=torch.float64, device="cuda")
    assert L.dss_dec_group_step_dev(g._h, tab, 0, losses.data_ptr(), None) == -1 and "sits out" in L.dss_last_error().decode()
    xd = _x(x).cuda()
    tab[0] = T._GroupTrial(xd.data_ptr(), 9, xd.data_ptr(), None, 0, 1e-3, 0.99, 1e-8)
    assert L.dss_dec_group_step_dev(g._h, tab, 0, losses.data_ptr(), None) == -1 and "9 frames" in L.dss_last_error().decode()
    tab[0] = T._GroupTrial(None, 7, xd.data_ptr(), None, 0, 1e-3, 0.99, 1e-8)
    assert L.dss_dec_group_step_dev(g._h, tab, 0, losses.data_ptr(), None) == -1 and "null frames" in L.dss_last_error().decode()
    # a member without parameters may sit out, not step
    raw = L.dss_dec_group_create(2, C, H, O, 8)
    assert raw
    try:
        tab[0] = T._GroupTrial(xd.data_ptr(), 7, xd.data_ptr(), None, 0, 1e-3, 0.99, 1e-8)
        assert L.dss_dec_group_step_dev(raw, tab, 0, losses.data_ptr(), None) == -1 and "no parameters loaded" in L.dss_last_error().decode()
    finally:
        L.dss_dec_group_destroy(raw)
    assert Ct.sizeof(T._GroupTrial) == 64
