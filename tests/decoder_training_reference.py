"""Float64 references for the decoder's training step (csrc/dec_train.hip), for tests: a helper module like
vad_training_reference.py.

* ``autograd_trial``: torch autograd in float64 over four single-direction single-layer ``nn.LSTM``s (the reverse ones run on the
  flipped sequence), the dropout mask multiplied into layer 0's concatenated output, then ``Linear`` and ``MSELoss`` -- the same
  ``state_dict`` as ``BidirectionalSpeechSynthesisModel``.  tests/test_cpu_decoder_training.py pins it to that class (float64,
  dropout 0: loss and all eighteen gradients within 1e-12).
* ``manual_trial``: the same trial written out in numpy (forward with a stash, backward through time in both directions), so that
  one defect of the kind a kernel could have can be injected (``DEFECTS``); without a defect it agrees with autograd to rounding.
* ``reference_loop``: the script's loop (train_bidirectional_model.py:134-152) on the float64 four-LSTM module with
  ``torch.optim.RMSprop`` and given masks.  ``rmsprop64`` is vad_training_reference's.
* the inputs of the GPU tests (``GRAD_CASES``, ``case_inputs``, ``learning_problem``, ``LEARN``), their bounds, and the checker
  that tests/test_gpu_decoder_training.py and tests/test_gpu_training_cases.py share (``check_trial``, ``loss_bound``).

GRAD_BOUND -- per tensor, max|g - g_f64| / max|g_f64| -- is 4 x the worst error of torch float32 CPU autograd against
``autograd_trial`` over GRAD_CASES (every case with and without a mask), rounded up to one significant digit;
tools/decoder_training_bounds.py measures it without a GPU.  The factor 4 covers a different summation order and different expf /
tanhf.  The torch figure behind the constant and the kernels' own figure on MI355X are beside it below."""
from __future__ import annotations

import numpy as np

import lstm_reference as R
from vad_training_reference import rmsprop64  # noqa: F401  (re-exported: the optimiser formula is the same)

KEYS = tuple(f"lstm.{n}_l{layer}{rev}" for layer in (0, 1) for rev in ("", "_reverse")
             for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) + ("regressor.weight", "regressor.bias")

# torch float32 CPU autograd, worst tensor over the cases: 1.48e-6 (lstm.weight_hh_l0 at (100, 64, 37) x 4 with a mask; 1.0e-6 at
# (100, 64, 2); 9.2e-7 at the 350-frame trial, which therefore needs no constant of its own);  x 4 = 5.9e-6 -> 6e-6.
# The kernels on MI355X, worst tensor over the same cases: 1.97e-6 (at (100, 64, 37) x 4; 8.5e-7 or less at every case of scale 1).
# The case table of tests/training_cases.py fits the same constant: torch float32 1.30e-6 at worst ((7, 5, 9) x 4 without a mask);
# the kernels on MI355X 1.52e-6 in a gradient ((6, 5, 513) with 20 outputs), 7.7e-9 in the loss, 1.9e-7 in the features at scale 4
# and 8.1e-8 at scale 1.
GRAD_BOUND = 6e-6

# (H, C, T, scale of the LSTM weights)
GRAD_CASES = ((100, 64, 1, 1), (100, 64, 2, 1), (100, 64, 3, 1), (100, 64, 4, 1), (100, 64, 5, 1), (6, 5, 7, 1), (100, 64, 50, 1),
              (128, 256, 9, 1), (100, 64, 37, 4), (100, 64, 350, 1))

DEFECTS = ("drop_dh_next_fwd", "drop_dh_next_bwd", "drop_dc_next_fwd", "drop_dc_next_bwd", "bwd_dG_at_forward_index",
           "mask_not_in_backward", "mask_halves_swapped", "dmid_misses_reverse_direction", "divisor_T_not_T_times_O",
           "hprev_of_bwd_from_wrong_side", "forget_gate_path_lost")


def _np64(sd):
    return {k: np.array(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64) for k, v in sd.items()}


def case_inputs(case, mask: str | None = "random", outputs: int | None = None):
    """The inputs of one gradient case: state_dict (float32 tensors, 20 outputs), x (T, C) float64 holding float32 values
    (N(0, 1) x 2), y (T, 20) float32 targets (N(0, 1)), mask (T, 2H) float32 multipliers of 0 / 2 or None.
    mask: None, "random", or "zero_row" (random with row T // 2 all zero).
    outputs: None leaves the state_dict's own 20-output regressor; a count draws a regressor of that many outputs at torch's
    default init of ``nn.Linear(2H, outputs)`` from a seed of the case's (tests/training_cases.py), and y is (T, outputs)."""
    H, C, T, scale = case
    sd = R.decoder_state_dict(H, C, scale)
    if outputs is not None:
        import torch
        torch.manual_seed(300 + 7 * H + outputs)
        head = torch.nn.Linear(2 * H, outputs)
        sd["regressor.weight"], sd["regressor.bias"] = head.weight.detach().clone(), head.bias.detach().clone()
    x = R.frames("x2", 1, T, C, 7100 + 13 * T + H)[0]
    rng = np.random.default_rng(9100 + 17 * T + H + scale)
    y = rng.standard_normal((T, sd["regressor.weight"].shape[0])).astype(np.float32)
    m = None
    if mask is not None:
        m = (rng.random((T, 2 * H)) >= 0.5).astype(np.float32) * np.float32(2.0)
        if mask == "zero_row":
            m[T // 2] = 0.0
    return sd, x, y, m


# ---- torch autograd ------------------------------------------------------------------------------------------------------------

def four_lstm_module(sd, dtype):
    """Four single-layer one-direction nn.LSTMs and the head, holding the parameters of `sd` in `dtype`; forward(x, mask)."""
    import torch
    import torch.nn as nn

    class FourLstm(nn.Module):
        def __init__(self, C, H, O):
            super().__init__()
            self.l0 = nn.LSTM(C, H, 1, batch_first=True)
            self.l0_reverse = nn.LSTM(C, H, 1, batch_first=True)
            self.l1 = nn.LSTM(2 * H, H, 1, batch_first=True)
            self.l1_reverse = nn.LSTM(2 * H, H, 1, batch_first=True)
            self.regressor = nn.Linear(2 * H, O)

        @staticmethod
        def _both(fwd, bwd, x):
            return torch.cat([fwd(x)[0], bwd(x.flip(1))[0].flip(1)], dim=2)

        def forward(self, x, mask=None):
            mid = self._both(self.l0, self.l0_reverse, x)
            if mask is not None:
                mid = mid * mask[None]
            return self.regressor(self._both(self.l1, self.l1_reverse, mid))

        def named(self):
            """The eighteen parameters under the names of BidirectionalSpeechSynthesisModel's state_dict."""
            out = {}
            for layer in (0, 1):
                for rev in ("", "_reverse"):
                    m = getattr(self, f"l{layer}{rev}")
                    for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                        out[f"lstm.{n}_l{layer}{rev}"] = getattr(m, n + "_l0")
            out["regressor.weight"], out["regressor.bias"] = self.regressor.weight, self.regressor.bias
            return out

    H4, C = sd["lstm.weight_ih_l0"].shape
    m = FourLstm(int(C), int(H4) // 4, int(sd["regressor.weight"].shape[0])).to(dtype)
    with torch.no_grad():
        for k, p in m.named().items():
            p.copy_(torch.as_tensor(np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k])).to(dtype))
    return m


def autograd_trial(sd, x, y, mask=None, dtype=None):
    """One trial by torch autograd (float64 unless dtype says otherwise): loss, {name: gradient}, features (T, O) -- all numpy."""
    import torch
    dtype = dtype or torch.float64
    m = four_lstm_module(sd, dtype)
    xt = torch.as_tensor(np.asarray(x)).to(dtype)[None]
    mk = None if mask is None else torch.as_tensor(np.asarray(mask)).to(dtype)
    out = m(xt, mk)
    loss = torch.nn.MSELoss(reduction="mean")(out, torch.as_tensor(np.asarray(y)).to(dtype)[None])
    loss.backward()
    grads = {k: p.grad.detach().numpy().astype(np.float64) for k, p in m.named().items()}
    return float(loss.detach()), grads, out.detach().numpy()[0].astype(np.float64)


# ---- the same trial written out, with one optional defect --------------------------------------------------------------------

def _sig(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def manual_trial(sd, x, y, mask=None, defect: str | None = None):
    """loss, {name: gradient}, features: forward with a stash, the mean squared error over T x O, backward through time; float64
    numpy.  Everything is indexed by FRAME; a direction's "step before" is frame t - 1 forward and t + 1 backward."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown defect {defect!r}")
    p = _np64(sd)
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    T = len(x)
    H = p["lstm.weight_hh_l0"].shape[1]
    O = p["regressor.weight"].shape[0]
    mk = np.ones((T, 2 * H)) if mask is None else np.asarray(mask, np.float64)
    sfx = ("", "_reverse")
    inp, stash = x, {}
    for layer in (0, 1):
        outs = []
        for d in (0, 1):
            wi, wh, bi, bh = (p[f"lstm.{n}_l{layer}{sfx[d]}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            h, c = np.zeros(H), np.zeros(H)
            act, hprev, cprev, cnew, hout = [None] * T, np.zeros((T, H)), np.zeros((T, H)), np.zeros((T, H)), np.zeros((T, H))
            for t in (range(T - 1, -1, -1) if d else range(T)):
                hprev[t], cprev[t] = h, c
                g = wi @ inp[t] + bi + wh @ h + bh
                i, f, gg, o = _sig(g[:H]), _sig(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), _sig(g[3 * H:])
                c = f * c + i * gg
                h = o * np.tanh(c)
                act[t], cnew[t], hout[t] = (i, f, gg, o), c, h
            stash[layer, d] = (inp, act, hprev, cprev, cnew, hout)
            outs.append(hout)
        inp = np.concatenate(outs, axis=1)
        if layer == 0:
            inp = inp * mk
    top = inp
    feat = top @ p["regressor.weight"].T + p["regressor.bias"]
    loss = float(np.mean((feat - y) ** 2))
    dfeat = 2.0 * (feat - y) / (T if defect == "divisor_T_not_T_times_O" else T * O)
    grads = {"regressor.weight": dfeat.T @ top, "regressor.bias": dfeat.sum(0)}
    up = dfeat @ p["regressor.weight"]                     # what arrives at layer 1's h from the head, per frame: (T, 2H)
    for layer in (1, 0):
        down = np.zeros((T, stash[layer, 0][0].shape[1]))
        for d in (0, 1):
            wi, wh = p[f"lstm.weight_ih_l{layer}{sfx[d]}"], p[f"lstm.weight_hh_l{layer}{sfx[d]}"]
            inp, act, hprev, cprev, cnew, hout = stash[layer, d]
            name = "bwd" if d else "fwd"
            dG = np.zeros((T, 4 * H))
            dhn, dcn = np.zeros(H), np.zeros(H)
            for t in (range(T) if d else range(T - 1, -1, -1)):       # the direction's own time, backwards
                i, f, gg, o = act[t]
                tc = np.tanh(cnew[t])
                dh = up[t, d * H:(d + 1) * H] + (0.0 if defect == f"drop_dh_next_{name}" else dhn)
                dc = dh * o * (1.0 - tc * tc) + (0.0 if defect == f"drop_dc_next_{name}" else dcn)
                df = np.zeros(H) if defect == "forget_gate_path_lost" else dc * cprev[t] * f * (1.0 - f)
                dG[t] = np.concatenate([dc * gg * i * (1.0 - i), df, dc * i * (1.0 - gg * gg), dh * tc * o * (1.0 - o)])
                dcn = dc * f
                dhn = wh.T @ dG[t]
            if d and defect == "bwd_dG_at_forward_index":
                dG = dG[::-1].copy()
            hp = hprev
            if d and defect == "hprev_of_bwd_from_wrong_side":
                hp = np.concatenate([np.zeros((1, H)), hout[:-1]])             # h of frame t - 1 instead of t + 1
            grads[f"lstm.weight_ih_l{layer}{sfx[d]}"] = dG.T @ inp
            grads[f"lstm.weight_hh_l{layer}{sfx[d]}"] = dG.T @ hp
            grads[f"lstm.bias_ih_l{layer}{sfx[d]}"] = dG.sum(0)
            grads[f"lstm.bias_hh_l{layer}{sfx[d]}"] = dG.sum(0)
            if not (d and defect == "dmid_misses_reverse_direction"):
                down = down + dG @ wi
        if layer == 1:
            if defect == "mask_halves_swapped":
                down = down * np.concatenate([mk[:, H:], mk[:, :H]], axis=1)
            elif defect != "mask_not_in_backward":
                down = down * mk
            up = down
    return loss, grads, feat


def rel_errors(got: dict, want: dict) -> dict:
    """Per tensor: max|got - want| / max|want|.  A tensor whose true gradient is all zero (weight_hh of a one-frame trial: the
    state before the only step is zero) must be zero: 0 if it is, inf if not."""
    out = {}
    for k in KEYS:
        diff, ref = float(np.abs(np.asarray(got[k], np.float64) - want[k]).max()), float(np.abs(want[k]).max())
        out[k] = diff / ref if ref > 0 else (0.0 if diff == 0 else float("inf"))
    return out


# ---- what the GPU tests hold a trial to ---------------------------------------------------------------------------------------

def loss_bound(feat64, y, scale):
    """loss = mean over the T x O elements of (f - y)^2.  With |f - f64| <= b = bound(scale) per element,
    |(f - y)^2 - (f64 - y)^2| = |f - f64| |(f - y) + (f64 - y)| <= b (2 |f64 - y| + b), so
    |loss - loss64| <= b (2 mean|f64 - y| + b): the loss's gradient in the features has L1 norm 2 mean|f64 - y|, the second term is
    the curvature.  The kernel's own sum is float64 over float32 features and adds nothing at this size."""
    b = R.bound(scale)
    return b * (2.0 * float(np.mean(np.abs(feat64 - np.asarray(y, np.float64)))) + b)


def check_trial(tr, sd, x, y, m, scale, f64_frames, what, want=None):
    """One ``trial(step=False)`` of the trainer ``tr`` (a DecoderTrainerGPU that holds ``sd``) against ``autograd_trial`` (or
    ``want``, its result): every gradient within GRAD_BOUND, the loss within ``loss_bound``, the features within
    lstm_reference.bound(scale).  Prints the figures, then asserts; returns (gradient, loss, feature) errors."""
    import torch
    xs = torch.from_numpy(x if f64_frames else x.astype(np.float32))
    loss = tr.trial(xs, y, mask=m, step=False)
    return compare_trial(tr, loss, y, scale, what, want or autograd_trial(sd, x, y, m))


def compare_trial(tr, loss, y, scale, what, want):
    """The read-backs of the trainer's last trial and its loss against ``want`` = (loss, gradients, features) in float64."""
    want_loss, want_g, want_f = want
    err = rel_errors(tr.gradients(), want_g)
    ef = float(np.abs(tr.features() - want_f).max())
    lb = loss_bound(want_f, y, scale)
    print(f"{what}: gradient {max(err.values()):.3g} ({max(err, key=err.get)}), loss {abs(loss - want_loss):.3g} (bound {lb:.3g}), "
          f"features {ef:.3g}")
    for k in KEYS:
        assert err[k] <= GRAD_BOUND, (what, k, err[k])
    assert abs(loss - want_loss) <= lb, (what, loss, want_loss)
    assert ef <= R.bound(scale), (what, ef)
    return max(err.values()), abs(loss - want_loss), ef


# ---- the script's loop -----------------------------------------------------------------------------------------------------------

def reference_loop(sd, trials, masks=None, lr=1e-4, epochs=1, order=None, on_epoch=None):
    """The script's loop in float64 on the four-LSTM module with torch.optim.RMSprop: trials = [(x (len, C), y (len, O))], masks =
    per epoch and trial a (len, 2H) array or None.  Returns (state_dict of float64 tensors, per-trial losses)."""
    import torch
    m = four_lstm_module(sd, torch.float64)
    named = m.named()
    optim = torch.optim.RMSprop(list(named.values()), lr=lr)
    cfunc = torch.nn.MSELoss(reduction="mean")
    losses = []
    for e in range(epochs):
        for k in (order or range(len(trials))):
            x, y = trials[k]
            xt = torch.as_tensor(np.asarray(x, np.float64))[None]
            yt = torch.as_tensor(np.asarray(y, np.float64))[None]
            mk = None if masks is None or masks[e][k] is None else torch.as_tensor(np.asarray(masks[e][k], np.float64))
            for q in named.values():
                q.grad = None
            loss = cfunc(m(xt, mk), yt)
            loss.backward()
            optim.step()
            losses.append(float(loss.detach()))
        if on_epoch is not None:
            on_epoch(e, {k: v.detach().clone() for k, v in named.items()})
    return {k: v.detach().clone() for k, v in named.items()}, losses


def validation_loss64(sd, trials):
    """The script's final_valid_loss: the mean over the trials of the per-trial mean squared error, float64, no dropout."""
    per = []
    for x, y in trials:
        f, _ = R.decoder_forward(sd, np.asarray(x, np.float64)[None])
        per.append(float(np.mean((f[0] - np.asarray(y, np.float64)) ** 2)))
    return float(np.mean(per))


# ---- the learning problem ------------------------------------------------------------------------------------------------------

LEARN = dict(H=16, C=8, O=4, lr=3e-3, dropout=0.5, epochs=5, seed=11)
# Validation loss after / before training on the learning problem.  The float64 reference_loop with LEARN's masks brings it to
# 0.196 (0.595, 0.377, 0.257, 0.223, 0.196 after the five epochs; lr and epochs were chosen so that it falls below 0.5).  The CPU
# test asserts that figure with a 10 % margin; the GPU test asserts it x 0.5 / 0.35 (the detector test's margin between the
# float64 run and the kernels' float32 run), and never more than 0.75.
LEARN_RATIO_F64 = 0.196
LEARN_RATIO_CPU = 1.1 * LEARN_RATIO_F64
LEARN_RATIO_GPU = min(0.75, LEARN_RATIO_F64 * 0.5 / 0.35)


def learning_problem():
    """state_dict (H 16, C 8, 4 outputs, default init), six trials of 90-140 frames of N(0, 1) (float32 values) whose targets are
    the centred 5-frame moving average of channels 0-2 (frames beyond the trial count as zero) through a fixed 3 x 4 matrix -- two
    frames of the past and two of the future, so both directions matter -- as [(x, y)] and as a corpus dict (hga_activity,
    lpc_coefficients, trial_ids)."""
    import torch
    rng = np.random.default_rng(2025)
    sd = R.decoder_state_dict(LEARN["H"], LEARN["C"], 1)
    torch.manual_seed(77)
    head = torch.nn.Linear(2 * LEARN["H"], LEARN["O"])
    sd["regressor.weight"], sd["regressor.bias"] = head.weight.detach().clone(), head.bias.detach().clone()
    mix = np.array([[1.0, -0.5, 0.25, 0.75], [-0.75, 1.0, 0.5, -0.25], [0.5, 0.25, -1.0, 1.0]])
    trials = []
    for k in range(6):
        n = int(rng.integers(90, 141))
        x = rng.standard_normal((n, LEARN["C"])).astype(np.float32).astype(np.float64)
        pad = np.concatenate([np.zeros((2, 3)), x[:, :3], np.zeros((2, 3))])
        avg = sum(pad[j:j + n] for j in range(5)) / 5.0
        trials.append((x, (avg @ mix).astype(np.float32)))
    corpus = dict(hga_activity=np.concatenate([x for x, _ in trials]), lpc_coefficients=np.concatenate([y for _, y in trials]),
                  trial_ids=np.concatenate([np.full(len(y), k) for k, (_, y) in enumerate(trials)]))
    return sd, trials, corpus


def learning_masks(trials):
    """The masks train_decoder draws for the learning problem (fixed trial order): per epoch and trial, from one generator seeded
    with LEARN['seed'], in the order of the calls."""
    import torch
    from dss_amd.training import decoder_dropout_mask
    gen = torch.Generator().manual_seed(LEARN["seed"])
    return [[decoder_dropout_mask(len(y), LEARN["H"], LEARN["dropout"], gen).numpy() for _, y in trials] for _ in range(LEARN["epochs"])]
