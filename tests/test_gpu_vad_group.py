"""Several detectors trained at once on the GPU (``VadGroupTrainerGPU`` / ``train_vads``, the group kernels of csrc/vad_train.hip)
against the single trainer (``VadTrainerGPU``), which tests/test_gpu_vad_training.py pins to float64 autograd.  For every model,
after every sequence of group steps, the per-window losses, the gradients, the square averages, the parameters and the carried
state are BIT-IDENTICAL (``np.array_equal`` on the raw arrays, no tolerance) to a single trainer loaded with the same weights and
given that model's trials in the same order -- whatever M is, wherever the model sits and whatever the other models do in the
same step.  One test holds the group path to ``V.autograd_window`` directly, with the single test's bounds.

Shapes: (H, C) = (6, 5), (150, 64) and (160, 128), the capacity corner; windows of 5 frames (one full chunk of VAD_TP = 4 frames
and a remainder); trials of at most 13 frames (two full windows and a remainder of 3)."""
import numpy as np
import pytest

import lstm_reference as R
import vad_training_reference as V

pytestmark = pytest.mark.gpu

W = 5


@pytest.fixture(scope="module")
def T():
    from dss_amd import training
    return training


def _member_sd(H, C, k):
    """Weights of member k: the precision tests' detector, moved by a seeded perturbation so that no two members are alike."""
    import torch
    sd = R.vad_state_dict(H, C, 1)
    if k:
        g = torch.Generator().manual_seed(4100 + k)
        sd = {n: v + 0.02 * torch.randn(v.shape, generator=g) for n, v in sd.items()}
    return sd


def _trial(H, C, n, seed, mask=True):
    """x (n, C) float64 holding float32 values, y (n,) uint8, mask (n, H) multipliers of 0 / 2 or None."""
    x = R.frames("x2", 1, n, C, 8700 + seed)[0]
    rng = np.random.default_rng(9700 + seed)
    y = rng.integers(0, 2, n).astype(np.uint8)
    m = (rng.random((n, H)) >= 0.5).astype(np.float32) * np.float32(2.0) if mask else None
    return x, y, m


def _x(x, f64=False):
    import torch
    return None if x is None else torch.from_numpy(x if f64 else x.astype(np.float32))


def _read(tr, m=None):
    """Every read-back of a single trainer (m None) or of member m of a group."""
    a = () if m is None else (m,)
    return tr.state_dict(*a), tr.gradients(*a), tr.square_avg(*a), tr.state(*a)


def _assert_same(got, want, what=""):
    for name, a, b in zip(("parameters", "gradients", "square averages"), got[:3], want[:3]):
        for k in V.KEYS:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, name, k)
    assert np.array_equal(got[3][0], want[3][0]) and np.array_equal(got[3][1], want[3][1]), (what, "state")


def _group_trials(g, step, f64=False, losses=None, **kw):
    """One trial step from [(x, y, mask) or None]; returns (losses as a host array, counts)."""
    out, counts = g.train_trials([None if s is None else _x(s[0], f64) for s in step], [None if s is None else s[1] for s in step], W,
                                 [None if s is None else s[2] for s in step], losses=losses, **kw)
    return out.cpu().numpy(), counts


def _run_both(T, sds, steps, f64=False, lr=1e-3):
    """steps[k][m] = (x, y, mask) or None.  Runs the group and M single trainers trial step by trial step; compares the losses of
    every window and all read-backs after every step.  Returns (group, single trainers)."""
    g = T.VadGroupTrainerGPU(sds, max_window=W)
    singles = [T.VadTrainerGPU(sd, max_window=W) for sd in sds]
    for k, step in enumerate(steps):
        losses, counts = _group_trials(g, step, f64, lr=lr)
        assert losses.shape == (len(sds), max(counts))
        for m, s in enumerate(step):
            if s is None:
                assert counts[m] == 0 and np.isnan(losses[m]).all()
                continue
            want = singles[m].train_trial(_x(s[0], f64), s[1], window=W, masks=s[2], lr=lr)
            assert counts[m] == len(want) == -(-len(s[1]) // W)
            assert np.array_equal(losses[m, :counts[m]], want), (k, m, losses[m], want)
            assert np.isnan(losses[m, counts[m]:]).all()
            _assert_same(_read(g, m), _read(singles[m]), f"step {k} model {m}")
    return g, singles


# ---- 1: the mixed trial step -------------------------------------------------------------------------------------------------------

MIX_LENGTHS = (13, 5, 11)         # two windows and a remainder of 3; exactly one window; two windows and a remainder of one frame


@pytest.mark.parametrize("f64", (False, True), ids=("float32 frames", "float64 frames"))
@pytest.mark.parametrize("H, C", [(6, 5), (150, 64), (160, 128)])
def test_mixed_trial_step_is_three_single_trainers(T, H, C, f64):
    sds = [_member_sd(H, C, m) for m in range(3)]
    steps = [[_trial(H, C, MIX_LENGTHS[(m + k) % 3], 10 * k + m + H) for m in range(3)] for k in range(2)]
    assert [len(s[1]) for s in steps[0]] == [13, 5, 11]
    g, singles = _run_both(T, sds, steps, f64=f64)
    # the state the step started from is not what it ends with, and the models differ
    assert g.state(0)[0].any() and not np.array_equal(g.state(0)[0], g.state(1)[0])


# ---- 2: the group path against float64 autograd -----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [V.GRAD_CASES[k] for k in (0, 3, 5, 6)], ids=str)
def test_group_window_against_float64_autograd(T, case):
    """Member 1 of a group of two, with a random mask, from a given state, step=False: gradients within V.GRAD_BOUND, loss within
    2 x R.bound, new h within R.bound, new c within R.C_REL -- the bounds of the single trainer's test; member 0 runs another
    window of another length beside it."""
    H, C, n, scale = case
    sd, x, y, state, m = V.case_inputs(case, "random")
    other = _trial(H, C, 3 if n != 3 else 4, 200 + n)
    g = T.VadGroupTrainerGPU([_member_sd(H, C, 1), sd], max_window=50)
    g.set_state(1, *state)
    before = g.state_dict(1)
    losses = g.window([_x(other[0]), _x(x)], [other[1], y], [other[2], m], step=False).cpu().numpy()
    want_loss, want, (wh, wc) = V.autograd_window(sd, x, y, state, m)
    err = V.rel_errors(g.gradients(1), want)
    h, c = g.state(1)
    eh, ec = np.abs(h - wh).max(), (np.abs(c - wc) / np.maximum(np.abs(wc), 1.0)).max()
    print(f"{case}: gradient {max(err.values()):.3g} ({max(err, key=err.get)}; bound {V.GRAD_BOUND:g}), loss {abs(losses[1] - want_loss):.3g} "
          f"(bound {2 * R.bound(scale):g}), h {eh:.3g} (bound {R.bound(scale):g}), c {ec:.3g} (bound {R.C_REL:g})")
    for k in V.KEYS:
        assert err[k] <= V.GRAD_BOUND, (k, err[k])
    assert abs(losses[1] - want_loss) <= 2 * R.bound(scale), (losses[1], want_loss)
    assert eh <= R.bound(scale) and ec <= R.C_REL, (eh, ec)
    assert all(np.array_equal(before[k].numpy(), g.state_dict(1)[k].numpy()) for k in V.KEYS)          # step=False
    # ... and it is the single trainer's window, bit for bit
    tr = T.VadTrainerGPU(sd, max_window=50)
    tr.set_state(*state)
    assert tr.window(_x(x), y, mask=m, step=False) == losses[1]
    _assert_same(_read(g, 1), _read(tr), "window")


# ---- 3: sitting out, and a trial that ends early ------------------------------------------------------------------------------------

def test_a_model_that_sits_out_or_whose_trial_ended_is_left_alone(T):
    import torch
    from dss_amd.vad import VadLstmGPU
    H, C = 6, 5
    sds = [_member_sd(H, C, m) for m in range(3)]
    first = [_trial(H, C, n, 300 + m) for m, n in enumerate((13, 11, 13))]
    second = [_trial(H, C, 13, 310), None, _trial(H, C, 13, 312)]
    third = [_trial(H, C, 13, 320), _trial(H, C, 3, 321), _trial(H, C, 13, 322)]
    g, singles = _run_both(T, sds, [first])
    before = _read(g, 1)
    assert before[1]["lstm.weight_hh_l0"].any() and before[2]["lstm.weight_hh_l0"].any() and before[3][0].any()
    det = VadLstmGPU(1, state_dict=sds[1])
    xs = torch.from_numpy(first[1][0].astype(np.float32)).cuda()[None]
    g.publish(1, det)
    _, packed_before = det.step_torch(xs, want_logits=True)
    packed_before = packed_before.clone()
    # a step it sits out: every slot of its row keeps the sentinel
    sentinel = torch.full((3, 3), 12345.0, dtype=torch.float64, device="cuda")
    got, counts = _group_trials(g, second, losses=sentinel, lr=1e-3)
    assert counts == [3, 0, 3] and (got[1] == 12345.0).all() and not (got[0] == 12345.0).any()
    _assert_same(_read(g, 1), before, "sat out")
    _assert_same(_read(g, 1), _read(singles[1]), "sat out, against the single trainer")
    det.reset()
    g.publish(1, det)
    assert torch.equal(det.step_torch(xs, want_logits=True)[1], packed_before)                            # the packed copies too
    for m in (0, 2):
        assert np.array_equal(got[m], singles[m].train_trial(_x(second[m][0]), second[m][1], window=W, masks=second[m][2], lr=1e-3))
    # a step in which its trial is one window long and the others' three: windows 1 and 2 leave it alone
    sentinel = torch.full((3, 4), 12345.0, dtype=torch.float64, device="cuda")
    got, counts = _group_trials(g, third, losses=sentinel, lr=1e-3)
    assert counts == [3, 1, 3] and got.shape == (3, 4)
    assert (got[1, 1:] == 12345.0).all() and (got[:, 3] == 12345.0).all()
    for m in range(3):
        want = singles[m].train_trial(_x(third[m][0]), third[m][1], window=W, masks=third[m][2], lr=1e-3)
        assert np.array_equal(got[m, :counts[m]], want), m
        _assert_same(_read(g, m), _read(singles[m]), f"third step, model {m}")


# ---- 4: position and width ---------------------------------------------------------------------------------------------------------

def _other_length(j, k, taken):
    """1 .. 13 frames, varying with the member and the step, never the length of the trial under test."""
    n = 1 + (5 * j + 3 * k + 1) % 13
    return n if n != taken else n % 13 + 1


def test_position_in_the_group_and_its_width_change_no_bit(T):
    H, C = 6, 5
    sd = _member_sd(H, C, 99)
    mine = [_trial(H, C, n, 400 + k) for k, n in enumerate((13, 4))]
    single = T.VadTrainerGPU(sd, max_window=W)
    want = []
    for x, y, m in mine:
        losses = single.train_trial(_x(x), y, window=W, masks=m, lr=1e-3)
        want.append((losses, _read(single)))
    for M, pos in ((1, 0), (3, 2), (5, 4), (64, 63)):
        sds = [_member_sd(H, C, m) for m in range(M)]
        sds[pos] = sd
        g = T.VadGroupTrainerGPU(sds, max_window=W)
        assert len(g) == M
        for k, (x, y, m) in enumerate(mine):
            others = {j: _trial(H, C, _other_length(j, k, len(y)), 1000 * k + j, mask=bool(j % 2)) for j in range(M) if j != pos}
            assert all(len(o[1]) <= 13 and len(o[1]) != len(y) for o in others.values())
            step = [(x, y, m) if j == pos else others[j] for j in range(M)]
            losses, counts = _group_trials(g, step, lr=1e-3)
            assert np.array_equal(losses[pos, :counts[pos]], want[k][0]), (M, k)
            _assert_same(_read(g, pos), want[k][1], f"M {M} step {k}")
            if M == 64 and k == 0:                         # every other member of the widest group, on its one trial
                for j, (ox, oy, om) in others.items():
                    tr = T.VadTrainerGPU(sds[j], max_window=W)
                    # (masks=None draws a mask in train_trial unless dropout is 0; in the group it is no mask)
                    assert np.array_equal(losses[j, :counts[j]], tr.train_trial(_x(ox), oy, window=W, dropout=0.0, masks=om, lr=1e-3)), j
                    _assert_same(_read(g, j), _read(tr), f"M = 64, member {j}")


# ---- 5: lr, alpha and eps per model --------------------------------------------------------------------------------------------------

def test_lr_alpha_eps_per_model(T):
    H, C = 6, 5
    sd = _member_sd(H, C, 7)                               # the same weights and trials: only the optimiser's numbers tell the models apart
    trials = [_trial(H, C, 13, 500 + k) for k in range(2)]
    lrs, alphas, epss = [1e-4, 3e-3, 1e-2], [0.99, 0.9, 0.95], [1e-8, 1e-6, 1e-3]
    g = T.VadGroupTrainerGPU([sd] * 3, max_window=W)
    singles = [T.VadTrainerGPU(sd, max_window=W) for _ in range(3)]
    for x, y, m in trials:
        losses, counts = _group_trials(g, [(x, y, m)] * 3, lr=lrs, alpha=alphas, eps=epss)
        for j in range(3):
            want = singles[j].train_trial(_x(x), y, window=W, masks=m, lr=lrs[j], alpha=alphas[j], eps=epss[j])
            assert np.array_equal(losses[j], want), j
            _assert_same(_read(g, j), _read(singles[j]), f"model {j}")
    a, b, c = (g.state_dict(j)["lstm.weight_ih_l0"].numpy() for j in range(3))
    assert not np.array_equal(a, b) and not np.array_equal(b, c)
    # one at a time: a scalar lr with alpha per model, then eps per model, against the matching single trainers
    g2 = T.VadGroupTrainerGPU([sd] * 2, max_window=W)
    x, y, m = trials[0]
    _group_trials(g2, [(x, y, m)] * 2, lr=1e-3, alpha=[0.99, 0.5])
    _group_trials(g2, [(x, y, m)] * 2, lr=1e-3, eps=[1e-8, 1e-2])
    for j, (al, ep) in enumerate(((0.99, 1e-8), (0.5, 1e-2))):
        tr = T.VadTrainerGPU(sd, max_window=W)
        tr.train_trial(_x(x), y, window=W, masks=m, lr=1e-3, alpha=al)
        tr.train_trial(_x(x), y, window=W, masks=m, lr=1e-3, eps=ep)
        _assert_same(_read(g2, j), _read(tr), f"alpha / eps, model {j}")


# ---- 6: back to back: the table ring wraps ----------------------------------------------------------------------------------------

def test_twelve_trial_steps_enqueued_back_to_back(T):
    """Twelve trial steps with twelve length tables, enqueued with nothing in between that waits for the device (frames, targets
    and masks are on the device before the first): the ring of eight tables wraps, and every step reads its own table."""
    import torch
    H, C, M = 6, 5, 3
    tables = [tuple(1 + (7 * k + 4 * m) % 13 if (k + m) % 5 else 0 for m in range(M)) for k in range(12)]
    assert all(any(t) for t in tables) and any(0 in t for t in tables)
    sds = [_member_sd(H, C, m) for m in range(M)]
    steps = [[_trial(H, C, n, 600 + 10 * k + m) if n else None for m, n in enumerate(tab)] for k, tab in enumerate(tables)]
    dev = [[None if s is None else (torch.from_numpy(s[0].astype(np.float32)).cuda(), torch.from_numpy(s[1]).cuda(), torch.from_numpy(s[2]).cuda())
            for s in step] for step in steps]
    g = T.VadGroupTrainerGPU(sds, max_window=W)
    torch.cuda.synchronize()
    out = [g.train_trials([s and s[0] for s in step], [s and s[1] for s in step], W, [s and s[2] for s in step], lr=1e-3) for step in dev]
    out = [(losses.cpu().numpy(), counts) for losses, counts in out]
    for m in range(M):
        tr = T.VadTrainerGPU(sds[m], max_window=W)
        for k, step in enumerate(steps):
            losses, counts = out[k]
            if step[m] is None:
                assert counts[m] == 0 and np.isnan(losses[m]).all()
            else:
                want = tr.train_trial(_x(step[m][0]), step[m][1], window=W, masks=step[m][2], lr=1e-3)
                assert np.array_equal(losses[m, :counts[m]], want), (k, m)
        _assert_same(_read(g, m), _read(tr), f"after twelve steps, model {m}")


# ---- 7: publish --------------------------------------------------------------------------------------------------------------------

def test_publish_of_a_member_then_validation_is_validation_of_its_state_dict(T):
    from dss_amd.vad import VadLstmGPU
    from dss_amd.validation import vad_validation
    sd, trials, corpus = V.learning_problem()
    H, C = V.LEARN["H"], V.LEARN["C"]
    g = T.VadGroupTrainerGPU([_member_sd(H, C, 1), sd], max_window=V.LEARN["window"])
    masks = V.learning_masks(trials)[0]
    for k in range(3):
        x, y = trials[k]
        g.train_trials([_x(trials[5 - k][0]), _x(x)], [trials[5 - k][1], y], V.LEARN["window"], [None, masks[k]], lr=V.LEARN["lr"])
    det = VadLstmGPU(1, state_dict=sd)
    g.publish(1, det)
    args = (corpus["hga_activity"], corpus["vad_labels"], corpus["trial_ids"])
    a, b, before, other = vad_validation(det, *args), vad_validation(g.state_dict(1), *args), vad_validation(sd, *args), vad_validation(g.state_dict(0), *args)
    assert np.array_equal(a["pred"], b["pred"]) and np.array_equal(a["prob"], b["prob"])
    assert np.array_equal(a["per_trial_loss"], b["per_trial_loss"]) and a["loss"] == b["loss"] and a["accuracy"] == b["accuracy"]
    assert not np.array_equal(a["prob"], before["prob"]) and not np.array_equal(a["prob"], other["prob"])
    with pytest.raises(Exception, match="inputs"):
        g.publish(1, VadLstmGPU(1, state_dict=R.vad_state_dict(6, 5, 1)))
    with pytest.raises(IndexError):
        g.publish(2, det)


# ---- 8: the epoch loops ------------------------------------------------------------------------------------------------------------

def _head(corpus, trials, n):
    rows = sum(len(y) for _, y in trials[:n])
    return {k: v[:rows] for k, v in corpus.items()}


@pytest.mark.parametrize("mask_source", ("host", "device"))
@pytest.mark.parametrize("shuffle, epochs", [(False, V.LEARN["epochs"]), (True, 2)])
def test_train_vads_is_train_vad_per_model(T, shuffle, epochs, mask_source):
    sd, trials, corpus = V.learning_problem()
    L = V.LEARN
    seeds = (11, 12, 13)
    sds = [sd, _member_sd(L["H"], L["C"], 1), sd]
    corpora = [corpus, corpus, _head(corpus, trials, 5)]   # model 2 sits out the last step of every epoch
    kw = dict(epochs=epochs, window=L["window"], dropout=L["dropout"], shuffle=shuffle, mask_source=mask_source)
    got = T.train_vads(sds, corpora, [corpus] * 3, lr=L["lr"], seeds=seeds, **kw)
    assert len(got) == 3
    windows = [sum(-(-len(y) // L["window"]) for _, y in trials[:n]) for n in (6, 6, 5)]
    for m in range(3):
        best, hist = T.train_vad(sds[m], corpora[m], corpus, lr=L["lr"], seed=seeds[m], **kw)
        assert got[m][1] == hist, (m, got[m][1], hist)
        assert [h["update_steps"] for h in hist] == [windows[m] * (e + 1) for e in range(epochs)]
        assert all(np.array_equal(got[m][0][k].numpy(), best[k].numpy()) for k in V.KEYS), m
    assert got[0][1] != got[2][1]


# ---- 9: refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(T):
    import torch
    from dss_amd import _lib
    H, C = 6, 5
    L = _lib.load()
    sds = [_member_sd(H, C, m) for m in range(2)]
    g = T.VadGroupTrainerGPU(sds, max_window=W)
    first = [_trial(H, C, 13, 900), _trial(H, C, 7, 901)]
    singles = [T.VadTrainerGPU(sd, max_window=W) for sd in sds]
    got, counts = _group_trials(g, first, lr=1e-3)
    for m in range(2):
        assert np.array_equal(got[m, :counts[m]], singles[m].train_trial(_x(first[m][0]), first[m][1], window=W, masks=first[m][2], lr=1e-3))
    before = [_read(g, m) for m in range(2)]

    x, y, mk = _trial(H, C, 4, 902)
    xd, yd = _x(x).cuda(), torch.from_numpy(y).cuda()
    losses = torch.full((2, 4), 777.0, dtype=torch.float64, device="cuda")
    entry = lambda n, frames=xd.data_ptr(), targets=yd.data_ptr(), out=losses.data_ptr(): T._VadGroupTrial(frames, targets, None, out, 1e-3, 0.99,
                                                                                                            1e-8, n, 1)

    def refused(call, *fragments):
        assert call() == -1
        msg = L.dss_last_error().decode()
        assert all(f in msg for f in fragments), msg

    tab = (T._VadGroupTrial * 2)()
    both = (lambda: L.dss_vad_group_window_dev(g._h, tab, 0, None), lambda: L.dss_vad_group_trial_dev(g._h, tab, W, 0, None))
    for call in both:
        tab[0], tab[1] = entry(0), entry(0)
        refused(call, "every model sits out")
        tab[1] = entry(-1)
        refused(call, "model 1", "-1 frames")
        tab[1] = entry(4, frames=None)
        refused(call, "model 1", "null frames, targets or losses")
        tab[1] = entry(4, targets=None)
        refused(call, "model 1", "null frames, targets or losses")
        tab[1] = entry(4, out=None)
        refused(call, "model 1", "null frames, targets or losses")
    tab[0], tab[1] = entry(4), entry(W + 1)
    refused(both[0], "model 1", f"a window of {W + 1} frames", f"max_window = {W}")
    tab[1] = entry(4)
    for bad in (0, -1, W + 1):
        refused(lambda: L.dss_vad_group_trial_dev(g._h, tab, bad, 0, None), f"windows of {bad} frames", f"max_window = {W}")
    # a member without parameters may sit out, not step
    raw = L.dss_vad_group_create(2, C, H, W)
    assert raw
    try:
        tab[0], tab[1] = entry(0), entry(4)
        refused(lambda: L.dss_vad_group_window_dev(raw, tab, 0, None), "model 1 has no parameters loaded")
        refused(lambda: L.dss_vad_group_trial_dev(raw, tab, W, 0, None), "model 1 has no parameters loaded")
    finally:
        L.dss_vad_group_destroy(raw)
    # the class's own refusals, in front of the C ABI's
    with pytest.raises(ValueError, match="6 frames"):
        g.window([_x(x), _x(first[1][0][:6])], [y, first[1][1][:6]])
    with pytest.raises(_lib.DssError, match="windows of 6 frames"):
        g.train_trials([_x(x), _x(x)], [y, y], window=6)
    with pytest.raises(ValueError, match="mask must be"):
        g.train_trials([_x(x), _x(x)], [y, y], W, [mk, np.zeros((4, H + 1), np.float32)])
    with pytest.raises(ValueError, match="every model sits out"):
        g.window([None, None], [None, None])
    with pytest.raises(ValueError, match="3 entries for 2 models"):
        g.train_trials([_x(x)] * 3, [y] * 3, W)
    with pytest.raises(ValueError, match="1 entries for 2 models"):
        g.train_trials([_x(x)] * 2, [y] * 2, W, eps=[1e-8])
    with pytest.raises(TypeError, match="one dtype"):
        g.window([_x(x), _x(x, True)], [y, y])
    with pytest.raises(ValueError, match="losses must be"):
        g.train_trials([_x(x)] * 2, [y] * 2, W, losses=torch.zeros((2, 0), dtype=torch.float64, device="cuda"))
    # nothing was launched: no read-back and no loss slot has changed
    torch.cuda.synchronize()
    assert (losses.cpu().numpy() == 777.0).all()
    for m in range(2):
        _assert_same(_read(g, m), before[m], f"after the refusals, model {m}")
    # and the next valid step is the single trainers'
    second = [_trial(H, C, 9, 910), _trial(H, C, 13, 911)]
    got, counts = _group_trials(g, second, lr=1e-3)
    for m in range(2):
        assert np.array_equal(got[m, :counts[m]], singles[m].train_trial(_x(second[m][0]), second[m][1], window=W, masks=second[m][2], lr=1e-3))
        _assert_same(_read(g, m), _read(singles[m]), f"after a valid step, model {m}")
