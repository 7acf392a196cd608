"""Float64 references for the detector's training step (csrc/vad_train.hip), for tests: a helper module like lstm_reference.py.

* ``autograd_window``: torch autograd in float64 over two single-layer ``nn.LSTM``s with the dropout mask multiplied in between,
  then ``Linear`` -- the same ``state_dict`` as ``UnidirectionalVoiceActivityDetector``.  tests/test_cpu_vad_training.py pins it
  to that class (float64, dropout 0: loss and all ten gradients within 1e-12).
* ``manual_window``: the same window written out in numpy (forward with a stash, backward through time), so that one defect of the
  kind a kernel could have can be injected (``DEFECTS``); without a defect it agrees with autograd to rounding.
* ``rmsprop64``: the RMSprop formula in float64 from given p, sq, g.
* ``reference_loop``: the script's loop (train_unidirectional_vad.py:144-175) on the float64 two-LSTM module with
  ``torch.optim.RMSprop`` and given masks.
* the inputs of the GPU tests (``GRAD_CASES``, ``case_inputs``, ``learning_problem``), their bounds, and the checkers that
  tests/test_gpu_vad_training.py and tests/test_gpu_training_cases.py share (``check_window``, ``check_trial_is_its_windows``).

GRAD_BOUND -- per tensor, max|g - g_f64| / max|g_f64| -- is 4 x the worst error of torch float32 CPU autograd against
``autograd_window`` over GRAD_CASES (every case with and without a mask, plus the zero-row mask and the one-class window), rounded up to one significant digit;
tools/vad_training_bounds.py measures it without a GPU.  The factor 4 covers a different summation order and different expf /
tanhf.  The torch figure behind the constant and the kernels' own figure on MI355X are beside it below."""
from __future__ import annotations

import numpy as np

import lstm_reference as R

KEYS = ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0",
        "lstm.weight_ih_l1", "lstm.weight_hh_l1", "lstm.bias_ih_l1", "lstm.bias_hh_l1",
        "classifier.weight", "classifier.bias")

# torch float32 CPU autograd, worst tensor over the cases: 1.44e-6 (lstm.bias_ih_l1 at (150, 64, 4), no mask; 1.38e-6 at
# (150, 64, 37) x 4);  x 4 = 5.74e-6 -> 6e-6.
# The kernels on MI355X, worst tensor over the same cases: 1.81e-6 (at (150, 64, 4); 1.25e-6 at (150, 64, 37) x 4).
# The case table of tests/training_cases.py fits the same constant: torch float32 1.32e-6 at worst ((159, 127, 5) without a mask);
# the kernels on MI355X 7.96e-7 in a gradient (the same entry), 9.9e-9 in the loss, 2.9e-7 in h and 3.6e-7 (relative) in c.
GRAD_BOUND = 6e-6

# (H, C, T, scale of the LSTM weights)
GRAD_CASES = ((150, 64, 50, 1), (150, 64, 1, 1), (150, 64, 3, 1), (150, 64, 4, 1), (150, 64, 5, 1), (6, 5, 7, 1), (160, 128, 50, 1),
              (150, 64, 37, 4))

DEFECTS = ("drop_dh_next_l0", "drop_dh_next_l1", "drop_dc_next_l0", "drop_dc_next_l1", "mask_not_in_backward", "divisor_max_window",
           "state_not_in_first_step", "forget_gate_path_lost", "no_gradient_through_wih1")


def _np64(sd):
    return {k: np.array(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64) for k, v in sd.items()}


def case_inputs(case, mask: str | None = "random", targets: str = "random"):
    """The inputs of one gradient case: state_dict (float32 tensors), x (T, C) float64 holding float32 values (N(0, 1) x 2), y (T,)
    uint8, state (h, c) [2][H] float32 (N(0, 0.3) / N(0, 0.5)), mask (T, H) float32 multipliers of 0 / 2 or None.
    mask: None, "random", or "zero_row" (random with row T // 2 all zero); targets: "random" or "one_class"."""
    H, C, T, scale = case
    sd = R.vad_state_dict(H, C, scale)
    x = R.frames("x2", 1, T, C, 7000 + 13 * T + H)[0]
    rng = np.random.default_rng(9000 + 17 * T + H + scale)
    h = (rng.standard_normal((2, H)) * 0.3).astype(np.float32)
    c = (rng.standard_normal((2, H)) * 0.5).astype(np.float32)
    y = rng.integers(0, 2, T).astype(np.uint8) if targets == "random" else np.ones(T, np.uint8)
    m = None
    if mask is not None:
        m = (rng.random((T, H)) >= 0.5).astype(np.float32) * np.float32(2.0)
        if mask == "zero_row":
            m[T // 2] = 0.0
    return sd, x, y, (h, c), m


# ---- torch autograd ------------------------------------------------------------------------------------------------------------

def two_lstm_module(sd, dtype):
    """Two single-layer nn.LSTMs and the head, holding the parameters of `sd` in `dtype`; forward(x, state, mask)."""
    import torch
    import torch.nn as nn

    class TwoLstm(nn.Module):
        def __init__(self, C, H):
            super().__init__()
            self.l0 = nn.LSTM(C, H, 1, batch_first=True)
            self.l1 = nn.LSTM(H, H, 1, batch_first=True)
            self.classifier = nn.Linear(H, 2)

        def forward(self, x, state, mask=None):
            h, c = state
            y0, (ha, ca) = self.l0(x, (h[0:1], c[0:1]))
            if mask is not None:
                y0 = y0 * mask[None]
            y1, (hb, cb) = self.l1(y0, (h[1:2], c[1:2]))
            return self.classifier(y1), (torch.cat([ha, hb]), torch.cat([ca, cb]))

        def named(self):
            """The ten parameters under the names of UnidirectionalVoiceActivityDetector's state_dict."""
            out = {}
            for layer, m in ((0, self.l0), (1, self.l1)):
                for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    out[f"lstm.{n}_l{layer}"] = getattr(m, n + "_l0")
            out["classifier.weight"], out["classifier.bias"] = self.classifier.weight, self.classifier.bias
            return out

    H4, C = sd["lstm.weight_ih_l0"].shape
    m = TwoLstm(int(C), int(H4) // 4).to(dtype)
    with torch.no_grad():
        for k, p in m.named().items():
            p.copy_(torch.as_tensor(np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k])).to(dtype))
    return m


def autograd_window(sd, x, y, state, mask=None, dtype=None):
    """One window by torch autograd (float64 unless dtype says otherwise): loss, {name: gradient}, (h, c) [2][H] -- all numpy."""
    import torch
    dtype = dtype or torch.float64
    m = two_lstm_module(sd, dtype)
    xt = torch.as_tensor(np.asarray(x)).to(dtype)[None]
    st = tuple(torch.as_tensor(np.asarray(s)).to(dtype)[:, None, :] for s in state)
    mk = None if mask is None else torch.as_tensor(np.asarray(mask)).to(dtype)
    out, (h, c) = m(xt, st, mk)
    loss = torch.nn.CrossEntropyLoss()(out.reshape(-1, 2), torch.as_tensor(np.asarray(y, dtype=np.int64)))
    loss.backward()
    grads = {k: p.grad.detach().numpy().astype(np.float64) for k, p in m.named().items()}
    return float(loss.detach()), grads, (h.detach().numpy()[:, 0].astype(np.float64), c.detach().numpy()[:, 0].astype(np.float64))


# ---- the same window written out, with one optional defect -------------------------------------------------------------------

def _sig(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def manual_window(sd, x, y, state, mask=None, defect: str | None = None, max_window: int = 50):
    """loss, {name: gradient}, (h, c): forward with a stash, cross-entropy (mean over T), backward through time; float64 numpy."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")
    p = _np64(sd)
    x = np.asarray(x, np.float64)
    T = len(x)
    H = p["lstm.weight_hh_l0"].shape[1]
    mk = np.ones((T, H)) if mask is None else np.asarray(mask, np.float64)
    inp, stash, hs, cs = x, [], [], []
    for layer in (0, 1):
        wi, wh, bi, bh = (p[f"lstm.{n}_l{layer}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
        h, c = np.array(state[0][layer], np.float64), np.array(state[1][layer], np.float64)
        hall, call, act = [h], [c], []
        for t in range(T):
            hin = np.zeros(H) if (defect == "state_not_in_first_step" and t == 0) else h
            g = wi @ inp[t] + bi + wh @ hin + bh
            i, f, gg, o = _sig(g[:H]), _sig(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), _sig(g[3 * H:])
            c = f * c + i * gg
            h = o * np.tanh(c)
            act.append((i, f, gg, o)); hall.append(h); call.append(c)
        stash.append((inp, np.array(hall), np.array(call), act))
        hs.append(h); cs.append(c)
        if layer == 0:
            inp = np.array(hall[1:]) * mk
    h1 = stash[1][1]
    z = h1[1:] @ p["classifier.weight"].T + p["classifier.bias"]
    lse = np.logaddexp(z[:, 0], z[:, 1])
    yi = np.asarray(y, np.int64)
    loss = float(np.mean(lse - z[np.arange(T), yi]))
    dl = np.exp(z - lse[:, None])
    dl[np.arange(T), yi] -= 1.0
    dl /= max_window if defect == "divisor_max_window" else T
    grads = {"classifier.weight": dl.T @ h1[1:], "classifier.bias": dl.sum(0)}
    dtop = dl @ p["classifier.weight"]                      # what arrives at layer 1's h from the head, per frame
    for layer in (1, 0):
        wi, wh = p[f"lstm.weight_ih_l{layer}"], p[f"lstm.weight_hh_l{layer}"]
        inp, hall, call, act = stash[layer]
        dG = np.zeros((T, 4 * H))
        dhn, dcn = np.zeros(H), np.zeros(H)
        for t in range(T - 1, -1, -1):
            i, f, gg, o = act[t]
            tc = np.tanh(call[t + 1])
            dh = dtop[t] + (0.0 if defect == f"drop_dh_next_l{layer}" else dhn)
            dc = dh * o * (1.0 - tc * tc) + (0.0 if defect == f"drop_dc_next_l{layer}" else dcn)
            df = np.zeros(H) if defect == "forget_gate_path_lost" else dc * call[t] * f * (1.0 - f)
            dG[t] = np.concatenate([dc * gg * i * (1.0 - i), df, dc * i * (1.0 - gg * gg), dh * tc * o * (1.0 - o)])
            dcn = dc * f
            dhn = wh.T @ dG[t]
        hprev = hall[:-1].copy()
        if defect == "state_not_in_first_step":
            hprev[0] = 0.0
        grads[f"lstm.weight_ih_l{layer}"] = dG.T @ inp
        grads[f"lstm.weight_hh_l{layer}"] = dG.T @ hprev
        grads[f"lstm.bias_ih_l{layer}"] = dG.sum(0)
        grads[f"lstm.bias_hh_l{layer}"] = dG.sum(0)
        if layer == 1:
            dtop = dG @ wi
            if defect != "mask_not_in_backward":
                dtop = dtop * mk
            if defect == "no_gradient_through_wih1":
                dtop = np.zeros_like(dtop)
    return loss, grads, (np.array(hs), np.array(cs))


def rel_errors(got: dict, want: dict) -> dict:
    """Per tensor: max|got - want| / max|want|.  A tensor whose true gradient is all zero (weight_hh of a one-frame window from
    the zero state) must be zero: 0 if it is, inf if not -- as decoder_training_reference.rel_errors has it."""
    out = {}
    for k in KEYS:
        diff, ref = float(np.abs(np.asarray(got[k], np.float64) - want[k]).max()), float(np.abs(want[k]).max())
        out[k] = diff / ref if ref > 0 else (0.0 if diff == 0 else float("inf"))
    return out


# ---- what the GPU tests hold a window and a trial to ------------------------------------------------------------------------

def check_window(tr, sd, x, y, state, m, scale, f64_frames, what, want=None):
    """One ``window(step=False)`` of the trainer ``tr`` (a VadTrainerGPU that holds ``sd``) from ``state`` against
    ``autograd_window`` (or ``want``, its result): every gradient within GRAD_BOUND, the loss within 2 x lstm_reference.bound(scale),
    the new h within bound(scale), the new c within C_REL.  Prints the figures, then asserts; returns (gradient, loss, h, c) errors."""
    import torch
    tr.set_state(*state)
    xs = torch.from_numpy(x if f64_frames else x.astype(np.float32))
    loss = tr.window(xs, y, mask=m, step=False)
    want_loss, want_g, (wh, wc) = want or autograd_window(sd, x, y, state, m)
    err = rel_errors(tr.gradients(), want_g)
    h, c = tr.state()
    eh, ec = float(np.abs(h - wh).max()), float((np.abs(c - wc) / np.maximum(np.abs(wc), 1.0)).max())
    print(f"{what}: gradient {max(err.values()):.3g} ({max(err, key=err.get)}), loss {abs(loss - want_loss):.3g}, h {eh:.3g}, c {ec:.3g}")
    for k in KEYS:
        assert err[k] <= GRAD_BOUND, (what, k, err[k])
    assert abs(loss - want_loss) <= 2 * R.bound(scale), (what, loss, want_loss)
    assert eh <= R.bound(scale) and ec <= R.C_REL, (what, eh, ec)
    return max(err.values()), abs(loss - want_loss), eh, ec


def check_trial_is_its_windows(training, H, C, n, window=50):
    """A trial of n frames through ``VadTrainerGPU.train_trial`` in windows of ``window`` frames (the trainer's ``max_window``),
    twice from the same loaded state, and once more window by window: ceil(n / window) losses, the same bits all three times
    (losses, parameters, square averages, carried state), and every window's gradients within GRAD_BOUND of autograd on the
    weights read back before it."""
    sd = R.vad_state_dict(H, C, 1)
    x = R.frames("x2", 1, n, C, 31 * n + H)[0]
    rng = np.random.default_rng(n + H)
    y = rng.integers(0, 2, n).astype(np.uint8)
    masks = (rng.random((n, H)) >= 0.5).astype(np.float32) * np.float32(2.0)
    lr = 1e-3
    runs = []
    for _ in range(2):                                     # the same trial twice from the same loaded state: the same bits
        tr = training.VadTrainerGPU(sd, max_window=window)
        tr.set_state(np.ones((2, H), np.float32), np.ones((2, H), np.float32))          # train_trial resets it
        losses = tr.train_trial(x, y, window=window, masks=masks, lr=lr)
        runs.append((losses, tr.state_dict(), tr.square_avg(), tr.state()))
    assert len(runs[0][0]) == -(-n // window)
    tr = training.VadTrainerGPU(sd, max_window=window)
    tr.set_state(np.ones((2, H), np.float32), np.ones((2, H), np.float32))
    tr.reset_state()
    seq = []
    for a in range(0, n, window):
        cur, state = tr.state_dict(), tr.state()
        seq.append(tr.window(x[a:a + window], y[a:a + window], mask=masks[a:a + window], step=True, lr=lr))
        _, want, _ = autograd_window(cur, x[a:a + window], y[a:a + window], state, masks[a:a + window])
        err = rel_errors(tr.gradients(), want)
        print(f"H {H} trial {n} window at {a}: gradient error {max(err.values()):.3g}")
        assert max(err.values()) <= GRAD_BOUND, (a, err)
    seq = (np.array(seq), tr.state_dict(), tr.square_avg(), tr.state())
    for other in (runs[1], seq):
        assert np.array_equal(runs[0][0], other[0])
        for k in KEYS:
            assert np.array_equal(runs[0][1][k].numpy(), other[1][k].numpy()), k
            assert np.array_equal(runs[0][2][k], other[2][k]), k
        assert np.array_equal(runs[0][3][0], other[3][0]) and np.array_equal(runs[0][3][1], other[3][1])


# ---- optimiser -----------------------------------------------------------------------------------------------------------------

def rmsprop64(p, sq, g, lr=1e-4, alpha=0.99, eps=1e-8):
    """torch.optim.RMSprop (momentum 0, not centred, no weight decay) on float64 copies of p, sq, g: (p', sq')."""
    p, sq, g = (np.asarray(a, np.float64) for a in (p, sq, g))
    sq2 = alpha * sq + (1.0 - alpha) * g * g
    return p - lr * g / (np.sqrt(sq2) + eps), sq2


def reference_loop(sd, trials, window=50, masks=None, lr=1e-4, epochs=1, order=None, on_epoch=None):
    """The script's loop in float64 on the two-LSTM module with torch.optim.RMSprop: trials = [(x (len, C), y (len,))], masks =
    per epoch and trial a (len, H) array or None.  Returns (state_dict of float64 tensors, per-window losses)."""
    import torch
    m = two_lstm_module(sd, torch.float64)
    named = m.named()
    optim = torch.optim.RMSprop(list(named.values()), lr=lr)
    cfunc = torch.nn.CrossEntropyLoss()
    H = named["lstm.weight_hh_l0"].shape[1]
    losses = []
    for e in range(epochs):
        for k in (order or range(len(trials))):
            x, y = trials[k]
            xt = torch.as_tensor(np.asarray(x, np.float64))[None]
            yt = torch.as_tensor(np.asarray(y, np.int64))
            mk = None if masks is None or masks[e][k] is None else torch.as_tensor(np.asarray(masks[e][k], np.float64))
            state = (torch.zeros((2, 1, H), dtype=torch.float64), torch.zeros((2, 1, H), dtype=torch.float64))
            for a in range(0, xt.shape[1], window):
                for q in named.values():
                    q.grad = None
                out, state = m(xt[:, a:a + window], state, None if mk is None else mk[a:a + window])
                loss = cfunc(out.reshape(-1, 2), yt[a:a + window])
                loss.backward()
                optim.step()
                state = (state[0].detach(), state[1].detach())
                losses.append(float(loss.detach()))
        if on_epoch is not None:
            on_epoch(e, {k: v.detach().clone() for k, v in named.items()})
    return {k: v.detach().clone() for k, v in named.items()}, losses


def validation_loss64(sd, trials):
    """The script's valid_loss (the sum of the per-trial cross-entropies) and accuracy, float64, no dropout."""
    tot, good, n = 0.0, 0, 0
    for x, y in trials:
        z, _ = R.vad_forward(sd, np.asarray(x, np.float64)[None])
        z = z[0]
        yi = np.asarray(y, np.int64)
        tot += float(np.mean(np.logaddexp(z[:, 0], z[:, 1]) - z[np.arange(len(yi)), yi]))
        good += int(((z[:, 1] > z[:, 0]).astype(np.int64) == yi).sum())
        n += len(yi)
    return tot, good / n


# ---- the learning problem ------------------------------------------------------------------------------------------------------

LEARN = dict(H=16, C=8, window=50, lr=1e-3, dropout=0.5, epochs=3, seed=11)


def learning_problem():
    """state_dict (H 16, C 8, default init), six trials of 90-140 frames of N(0, 1) with a 50-frame speech stretch whose first
    three channels are raised by 2 (float32 values), as [(x, y)] and as a corpus dict (hga_activity, vad_labels, trial_ids)."""
    rng = np.random.default_rng(2024)
    sd = R.vad_state_dict(LEARN["H"], LEARN["C"], 1)
    trials = []
    for k in range(6):
        n = int(rng.integers(90, 141))
        x = rng.standard_normal((n, LEARN["C"]))
        a = int(rng.integers(10, n - 60))
        y = np.zeros(n, np.uint8)
        y[a:a + 50] = 1
        x[a:a + 50, :3] += 2.0
        trials.append((x.astype(np.float32).astype(np.float64), y))
    corpus = dict(hga_activity=np.concatenate([x for x, _ in trials]), vad_labels=np.concatenate([y for _, y in trials]),
                  trial_ids=np.concatenate([np.full(len(y), k) for k, (_, y) in enumerate(trials)]))
    return sd, trials, corpus


def learning_masks(trials):
    """The masks train_vad draws for the learning problem (fixed trial order): per epoch and trial, from one generator seeded with
    LEARN['seed'], in the order of the calls."""
    import torch
    from dss_amd.training import dropout_mask
    gen = torch.Generator().manual_seed(LEARN["seed"])
    return [[dropout_mask(len(y), LEARN["H"], LEARN["dropout"], gen).numpy() for _, y in trials] for _ in range(LEARN["epochs"])]
