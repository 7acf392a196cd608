"""Float64 restatements of the two recurrent models of the online path, for tests (a helper module like oracle_api.py).

Plain numpy, written from dss_amd/models.py (torch.nn.LSTM's equations, gate order i, f, g, o):

    g = W_ih x_t + b_ih + W_hh h + b_hh;  i, f, o = sigmoid(.), g = tanh(.);  c' = f c + i g;  h' = o tanh(c')

* ``decoder_forward``: ``BidirectionalSpeechSynthesisModel.forward`` -- 2 layers, both directions, zero initial state, a
  layer's input at frame t is [h_forward(t), h_backward(t)] of the layer below, then Linear(2H -> O).  Optional per-stream
  lengths (the ragged call): the backward direction starts at the stream's own last frame, outputs beyond it are zero.
* ``vad_forward``: ``UnidirectionalVoiceActivityDetector.forward`` -- 2 layers, one direction, (h, c) carried in and out,
  then Linear(H -> 2).

Both take any ``state_dict`` (torch tensors or arrays), are batched over streams and step time in a Python loop.
``with_defect`` returns the network with one defect of the kind a kernel could have, for the power checks of the suite: a
test that cannot tell the defective network from the true one at its bound cannot catch that defect in a kernel either."""
from __future__ import annotations

import copy

import numpy as np

DEFECTS = ("whh_last_column", "first_step_bias", "tail_reads_previous")


class Net:
    """A state_dict as float64 arrays, plus at most one injected defect (``with_defect``)."""

    def __init__(self, state_dict):
        self.p = {k: np.array(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64)
                  for k, v in state_dict.items()}
        self.defect = None

    @property
    def H(self) -> int:
        return self.p["lstm.weight_hh_l0"].shape[1]

    def lstm(self, layer: int, reverse: bool = False):
        sfx = f"_l{layer}" + ("_reverse" if reverse else "")
        return tuple(self.p[f"lstm.{n}{sfx}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


def as_net(model) -> Net:
    return model if isinstance(model, Net) else Net(model)


def with_defect(model, kind: str, layer: int = 0, reverse: bool = False, row: int | None = None) -> Net:
    """The network of `model` (a state_dict or a Net) with one defect in LSTM layer `layer`, direction `reverse`:

    * ``whh_last_column``: W_hh[row, H-1] = 0 -- one weight of the last column, the one a kernel's zero-padded copy of W_hh
      (input counts rounded up to multiples of 4) holds in its last group; `row` defaults to unit H-1's forget gate.
    * ``first_step_bias``: b_ih[row] is left out on the first step only; `row` defaults to unit 0's cell gate.
    * ``tail_reads_previous``: when the frame count is not a multiple of 4, the last step of the layer reads the input of
      the step before it (a chunk of 4 steps whose tail indexes one frame short); in the backward direction that step is
      frame 0 and it reads frame 1.
    """
    if kind not in DEFECTS:
        raise ValueError(f"unknown defect {kind!r}: one of {DEFECTS}")
    net = copy.deepcopy(as_net(model))
    H = net.H
    if row is None:
        row = {"whh_last_column": H + H - 1, "first_step_bias": 2 * H, "tail_reads_previous": 0}[kind]
    if kind == "whh_last_column":
        sfx = f"_l{layer}" + ("_reverse" if reverse else "")
        net.p[f"lstm.weight_hh{sfx}"][row, H - 1] = 0.0
    else:
        net.defect = (kind, layer, reverse, row)
    return net


def _sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))                  # = 1 / (1 + exp(-x)), without overflow warnings


def lstm_layer(net: Net, layer: int, x, h0=None, c0=None, reverse: bool = False, lengths=None):
    """One LSTM layer over x (S, T, Cin) float64.  Returns y (S, T, H) (zero beyond a stream's length), h (S, H), c (S, H).
    lengths: per-stream frame counts (None: all T); the backward direction of stream s starts at frame lengths[s] - 1."""
    w_ih, w_hh, b_ih, b_hh = net.lstm(layer, reverse)
    S, T, _ = x.shape
    H = w_hh.shape[1]
    L = np.full(S, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    h = np.zeros((S, H)) if h0 is None else np.array(h0, np.float64)
    c = np.zeros((S, H)) if c0 is None else np.array(c0, np.float64)
    xw = x @ w_ih.T + (b_ih + b_hh)                        # input halves and biases of all steps at once
    whh_t = np.ascontiguousarray(w_hh.T)
    y = np.zeros((S, T, H))
    d = net.defect if net.defect is not None and net.defect[1] == layer and net.defect[2] == reverse else None
    rows = np.arange(S)
    for k in range(int(L.max()) if S else 0):
        live = k < L
        t = np.where(reverse, L - 1 - k, k).clip(0, T - 1)
        src = t
        if d is not None and d[0] == "tail_reads_previous":
            tail = live & (L % 4 != 0) & (k == L - 1) & (L >= 2)
            src = np.where(tail, np.where(reverse, t + 1, t - 1), t)
        g = xw[rows, src] + h @ whh_t
        if d is not None and d[0] == "first_step_bias" and k == 0:
            g[:, d[3]] -= b_ih[d[3]]
        i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
        cn = f * c + i * gg
        hn = o * np.tanh(cn)
        m = live[:, None]
        c = np.where(m, cn, c)
        h = np.where(m, hn, h)
        y[rows[live], t[live]] = hn[live]
    return y, h, c


def decoder_forward(model, x, lengths=None):
    """BidirectionalSpeechSynthesisModel.forward from the zero state: x (S, T, C) -> features (S, T, O) float64 (zero beyond a
    stream's length) and the final state (h, c), each [layer * 2 + direction][S][H] like torch.nn.LSTM's."""
    net = as_net(model)
    inp = np.asarray(x, np.float64)
    hs, cs = [], []
    for layer in (0, 1):
        yf, hf, cf = lstm_layer(net, layer, inp, lengths=lengths)
        yb, hb, cb = lstm_layer(net, layer, inp, reverse=True, lengths=lengths)
        inp = np.concatenate([yf, yb], axis=2)
        hs += [hf, hb]
        cs += [cf, cb]
    out = inp @ net.p["regressor.weight"].T + net.p["regressor.bias"]
    if lengths is not None:
        out[np.arange(inp.shape[1])[None, :] >= np.asarray(lengths)[:, None]] = 0.0
    return out, (np.stack(hs), np.stack(cs))


def vad_forward(model, x, state=None):
    """UnidirectionalVoiceActivityDetector.forward: x (S, T, C), state (h, c) each [2][S][H] (None: zeros) -> logits (S, T, 2)
    float64 and the new state.  Calling it packet by packet with the state carried gives what one call on the whole gives."""
    net = as_net(model)
    inp = np.asarray(x, np.float64)
    hs, cs = [], []
    for layer in (0, 1):
        h0, c0 = (None, None) if state is None else (state[0][layer], state[1][layer])
        inp, h, c = lstm_layer(net, layer, inp, h0, c0)
        hs.append(h)
        cs.append(c)
    return inp @ net.p["classifier.weight"].T + net.p["classifier.bias"], (np.stack(hs), np.stack(cs))


def scaled(state_dict, factor: float):
    """A copy of `state_dict` with every LSTM parameter (weights and biases, not the head) times `factor`: at 4x the gates leave
    0.5 and the cell state keeps memory over many frames, which default-init weights (|w| <= 1/sqrt(H)) barely do."""
    out = {}
    for k, v in state_dict.items():
        v = v.detach().clone() if hasattr(v, "detach") else np.array(v)
        out[k] = v * factor if k.startswith("lstm.") else v
    return out


# ---- the inputs of the float64 precision tests (tests/test_gpu_lstm_precision.py); the power checks of
# ---- tests/test_cpu_lstm_reference.py run on the same ones

BOUND = 2e-6          # |kernel - float64| of outputs (features, logits) and h, absolute, default-init weights
BOUND_X4 = 5e-5       # the same with the LSTM weights x4 (see bound())
C_REL = 1e-5          # |c_kernel - c_float64| <= C_REL * max(|c_float64|, 1)


def bound(scale: int) -> float:
    """The absolute bound on outputs and h for weights at `scale` x default init.

    Default init: 2e-6.  Measured on MI355X, the kernels' largest error against float64 over every case of the GPU tests is
    6.6e-7 (decoder features) / 3e-7 (VAD logits) / 1.6e-6 (VAD h, x30 frames), torch.nn.LSTM float32 on the same GPU 6.7e-7 /
    1.4e-7 / 1.5e-6.

    Weights x4: 5e-5.  These weights make the recurrence sensitive: over 2000 frames of constant or zero input, where nothing
    pulls the state back, float32 rounding is amplified, and torch float32 on the GPU is off by up to 1.8e-5 itself (kernel
    2.8e-5, both at the decoder's H 128 / C 256); x30 frames through C = 256 inputs put |W x| near 100, whose float32
    rounding alone reaches 4e-6 on the features after a few steps (kernel 4.7e-6, torch 4.6e-6); VAD h 6.2e-6 (torch 2.9e-6).
    The power checks (tests/test_cpu_lstm_reference.py) hold per defect: on the tests' own inputs each one moves the outputs
    by more than 10 x the bound of at least one weight set (the default-init run always; at x4 every defect but the decoder's
    first-step bias, which moves its features by 4 x 5e-5 there)."""
    return BOUND if scale == 1 else BOUND_X4
KINDS = ("x2", "x30", "constant", "zero")


def frames(kind: str, S: int, T: int, C: int, seed: int):
    """(S, T, C) frames, float64 holding float32 values (what the kernels compute on: they cast frames to float32 like the
    reference's units do).  x2 / x30: N(0, 1) times 2 / 30 (x30 saturates the gates); constant: one N(0, 1) x 2 frame per
    stream, repeated; zero: all zeros."""
    rng = np.random.default_rng(seed)
    if kind == "x2":
        x = rng.standard_normal((S, T, C)) * 2.0
    elif kind == "x30":
        x = rng.standard_normal((S, T, C)) * 30.0
    elif kind == "constant":
        x = np.repeat(rng.standard_normal((S, 1, C)) * 2.0, T, axis=1)
    elif kind == "zero":
        x = np.zeros((S, T, C))
    else:
        raise ValueError(kind)
    return x.astype(np.float32).astype(np.float64)


def decoder_state_dict(H: int, C: int, scale: float):
    """The decoder of the precision tests: BidirectionalSpeechSynthesisModel(2, H, C) at torch's default init (seed 0 for the
    reference's own 100 x 64, the golden vector's weights; 200 + H otherwise), LSTM parameters times `scale`."""
    import torch
    from dss_amd.models import BidirectionalSpeechSynthesisModel
    torch.manual_seed(0 if (H, C) == (100, 64) else 200 + H)
    return scaled(BidirectionalSpeechSynthesisModel(nb_layer=2, nb_hidden_units=H, nb_electrodes=C).eval().state_dict(), scale)


def vad_state_dict(H: int, C: int, scale: float):
    """The detector of the precision tests: UnidirectionalVoiceActivityDetector(2, H, C) at default init (seed 1 for 150 x 64, the
    golden vector's weights; 100 + H otherwise), LSTM parameters times `scale`."""
    import torch
    from dss_amd.models import UnidirectionalVoiceActivityDetector
    torch.manual_seed(1 if (H, C) == (150, 64) else 100 + H)
    return scaled(UnidirectionalVoiceActivityDetector(nb_layer=2, nb_hidden_units=H, nb_electrodes=C).eval().state_dict(), scale)


def decoder_cases(H: int, C: int):
    """(S, T, kind, float64 frames?, seed) of the plain decoder test at (H, C): every T of {1, 2, 3, 4, 5, 350, 2000} with every
    input kind (two streams), every S of {1, 128, 129, 256, 257, 1024} (so W = 1, 2 and 4, and last workgroups partly empty),
    and for (128, 256) also S = 200 (W = 2) and 300 (W = 4) at T = 350."""
    cases = []
    for T in (1, 2, 3, 4, 5, 350, 2000):
        for j, kind in enumerate(KINDS):
            cases.append((2, T, kind, (T + j) % 2 == 0, 1000 * T + j))
    for j, S in enumerate((1, 128, 129, 256, 257, 1024)):
        cases.append((S, 5, KINDS[j % 2], j % 2 == 0, 7 * S))
    if (H, C) == (128, 256):
        cases += [(200, 350, "x2", False, 200), (300, 350, "x30", True, 300)]
    return cases


def sample_streams(S: int, n_edge: int = 4):
    """The streams whose float64 reference a test computes when S is large (streams are independent): the first and last
    n_edge and n_edge from the middle, so every slot of a W = 2 / 4 workgroup and the partly empty last workgroup are seen."""
    m = (S // 2) & ~3
    return sorted(set(range(min(S, n_edge))) | set(range(max(0, S - n_edge), S)) | set(range(m, min(S, m + n_edge))))


def vad_packets(n_frames: int, seed: int):
    """Packet sizes summing to n_frames: mostly 4 (one amplifier packet), now and then 1 or 5."""
    rng = np.random.default_rng(seed)
    sizes, left = [], n_frames
    while left:
        w = min(left, int(rng.choice([4, 4, 4, 4, 4, 4, 1, 5])))
        sizes.append(w)
        left -= w
    return sizes


def ragged_case(scale: int):
    """The ragged decoder test's call: 257 segments (so workgroups carry W = 4) whose first workgroup holds 2000, 1, 0 and 777
    frames and the rest 0 ... 8, at scattered rows of a pool of N(0, 1) x 2 frames with 2100 frames per row (more than the
    call's 2000).  Returns counts, rows, pool (float64 holding float32 values)."""
    n = 257
    rng = np.random.default_rng(50 + scale)
    counts = rng.integers(0, 9, n)
    counts[:4] = (2000, 1, 0, 777)
    rows = rng.permutation(n + 7)[:n]
    return counts, rows, frames("x2", n + 7, 2100, 64, 60 + scale)
