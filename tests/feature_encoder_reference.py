"""The LPC feature encoder's binding definition: a float64 numpy statement of the method.

One fresh encoder per trial: ``n`` int16 samples give ``n // 160`` frames of 36 float32 outputs -- 18 Bark cepstral
coefficients, the pitch feature (18), the pitch correlation (19) and 16 LPC taps (20..35).  The structure follows xiph's
single-frame encoder as far as that is public knowledge; parity with xiph's code is NOT pinned (no copy of it is at hand).
What is pinned are the parts (tests/test_cpu_feature_encoder.py): the spectrum against numpy's FFT, the DCT against scipy,
the round trip through the decoder's inverse, the band partition, the floor, the pitch track on pulse trains, the whitening.

Everything is float64 except the float32 tables (window, DCT) and the LPC chain, which is the decoder's own
lpc_from_cepstrum in fp32, handed in as ``lpc_fn`` (the tests pass the checker's ``oracle.lpc_from_cepstrum``).

Sums whose order the kernels share term for term are written as explicit loops (DCT, residual, track): with equal inputs both
sides then produce equal bits, which is what makes the all-zero trial exact.  A detail the band partition needs: bin 160, the
last band edge, is no band's interior; it goes wholly to band 17, so that the weights sum to 1 at every bin 0..160.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

FRAME = 160
WINDOW = 320
NB_BANDS = 18
LPC_ORDER = 16
N_OUT = 36
N_LAGS = 256             # score indices q = 0..255, lag 256 - q
N_TRACK = 224            # indices the pitch track follows (lags 33..256)
PREEMPHASIS = float(np.float32(0.85))
EDGES = 4 * np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40])
G_COLUMN = 255           # the score rows keep the sub-frame weight where lag 1 would stand (nothing reads lag 1)


def window_table() -> np.ndarray:
    """float32 [320]: sin(.5 pi sin^2(.5 pi (k + .5) / 160)), mirrored."""
    k = np.arange(FRAME, dtype=np.float64)
    half = np.sin(.5 * np.pi * np.sin(.5 * np.pi * (k + .5) / FRAME) ** 2)
    return np.concatenate([half, half[::-1]]).astype(np.float32)


def dct_table() -> np.ndarray:
    """float32 [18][18]: cos((i + .5) j pi / 18), column 0 times sqrt(.5) (the decoder's table)."""
    i = np.arange(NB_BANDS, dtype=np.float64)[:, None]
    j = np.arange(NB_BANDS, dtype=np.float64)[None, :]
    d = np.cos((i + .5) * j * np.pi / NB_BANDS)
    d[:, 0] *= np.sqrt(.5)
    return d.astype(np.float32)


def band_weights() -> np.ndarray:
    """[18][161]: the triangular partition before the two edge doublings."""
    w = np.zeros((NB_BANDS, WINDOW // 2 + 1))
    for i in range(NB_BANDS - 1):
        width = EDGES[i + 1] - EDGES[i]
        for j in range(width):
            frac = j / width
            w[i, EDGES[i] + j] += 1 - frac
            w[i + 1, EDGES[i] + j] += frac
    w[NB_BANDS - 1, EDGES[-1]] += 1.0
    return w


_W32 = window_table().astype(np.float64)
_D32 = dct_table().astype(np.float64)
_BW = band_weights()
_k = np.arange(WINDOW)[:, None] * np.arange(WINDOW // 2 + 1)[None, :]
_DFT = np.exp(-2j * np.pi * (_k % WINDOW) / WINDOW)
_PEN = np.array([0.02 * float(d * d) for d in range(-4, 5)])


def preemphasis(s: np.ndarray) -> np.ndarray:
    s = np.asarray(s).astype(np.float64)
    x = s.copy()
    x[1:] = s[1:] + (-PREEMPHASIS) * s[:-1]
    return x


def windowed_frames(x: np.ndarray, n_frames: int) -> np.ndarray:
    """(F, 320): x[160 i - 160 .. 160 i + 160) times the window, zeros before the trial."""
    pad = np.concatenate([np.zeros(FRAME), x[:FRAME * n_frames]])
    idx = FRAME * np.arange(n_frames)[:, None] + np.arange(WINDOW)[None, :]
    return pad[idx] * _W32 if n_frames else np.zeros((0, WINDOW))


def spectrum(xw: np.ndarray) -> np.ndarray:
    """(F, 161) complex: X[b] = (1/320) sum_k xw[k] exp(-2 pi i b k / 320)."""
    return (xw @ _DFT) / WINDOW


def band_energies(X: np.ndarray) -> np.ndarray:
    E = (X.real ** 2 + X.imag ** 2) @ _BW.T
    E[:, 0] *= 2
    E[:, NB_BANDS - 1] *= 2
    return E


def log_floor(E: np.ndarray) -> np.ndarray:
    Ly = np.empty_like(E)
    log_max = np.full(len(E), -2.0)
    follow = np.full(len(E), -2.0)
    for i in range(NB_BANDS):
        v = np.log10(1e-2 + E[:, i])
        v = np.maximum(log_max - 8, np.maximum(follow - 2.5, v))
        Ly[:, i] = v
        log_max = np.maximum(log_max, v)
        follow = np.maximum(follow - 2.5, v)
    return Ly


def dct(Ly: np.ndarray, table: np.ndarray | None = None) -> np.ndarray:
    """c[j] = sqrt(2/18) sum_i Ly[i] D[i][j], the terms added in ascending i (no c[0] offset here).  ``table``: another D than
    the float32 one (the tests' closed form in float64)."""
    D = _D32 if table is None else table
    s = np.zeros_like(Ly)
    for i in range(NB_BANDS):
        s = s + Ly[:, i:i + 1] * D[i][None, :]
    return s * np.sqrt(2. / NB_BANDS)


def cepstrum(x: np.ndarray, n_frames: int) -> np.ndarray:
    """float64 (F, 18): outputs 0..17 before the rounding to float32."""
    c = dct(log_floor(band_energies(spectrum(windowed_frames(x, n_frames)))))
    c[:, 0] -= 4
    return c


def residual(x: np.ndarray, lpc: np.ndarray, n_frames: int) -> np.ndarray:
    """e over t = -80 .. 160 F - 80 (index k is t + 80): the sample's own frame (t + 80) // 160 supplies the taps."""
    n = FRAME * n_frames
    xs = np.concatenate([np.zeros(80 + LPC_ORDER), x[:max(n - 80, 0)]])        # xs[m] = x[m - 96]
    own = np.arange(n) // FRAME
    a = np.asarray(lpc, dtype=np.float64)
    r = xs[LPC_ORDER:LPC_ORDER + n].copy()
    for j in range(LPC_ORDER):
        r = r + a[own, j] * xs[LPC_ORDER - 1 - j:LPC_ORDER - 1 - j + n]
    e = r.copy()
    e[1:] = r[1:] + 0.7 * r[:-1]
    return e


@dataclass
class Margin:
    """Smallest |a - b| over the strict comparisons and argmax gaps met, exact ties left out: a tie is decided by the stated
    rule (no damping, keep the earlier candidate, first index), and both sides meet it only where the operands are exact."""
    value: float = np.inf

    def take(self, diff):
        d = np.abs(np.asarray(diff, dtype=np.float64))
        d = d[d > 0]
        if d.size:
            self.value = min(self.value, float(d.min()))


def subframe_scores(e: np.ndarray, n_frames: int, margin: Margin | None = None) -> np.ndarray:
    """(2 F, 256): xc after damping at columns 0..254, the normalised sub-frame weight g at column 255."""
    S = 2 * n_frames
    out = np.zeros((S, N_LAGS))
    if not S:
        return out
    pad = np.concatenate([np.zeros(N_LAGS), e])
    W = np.lib.stride_tricks.sliding_window_view(pad, 80)
    q = np.arange(192)
    h1, h2, h3 = (256 + q) // 2, (256 + q + 2) // 2, (256 + q - 1) // 2
    g = np.zeros(S)
    for sf in range(S):
        B = W[80 * sf:80 * sf + N_LAGS]
        A = W[80 * sf + N_LAGS]
        aa = float(A @ A)
        xc = 2 * (B @ A) / np.maximum(1.0, 1 + aa + np.einsum("ij,ij->i", B, B))
        h = np.maximum(np.maximum(xc[h1], xc[h2]), xc[h3])
        if margin is not None:
            margin.take(xc[:192] - 1.1 * h)
        damp = xc[:192] < 1.1 * h
        xc = xc.copy()
        xc[:192][damp] *= 0.8
        out[sf] = xc
        g[sf] = aa
    for i in range(n_frames):
        tot = g[2 * i] + g[2 * i + 1] + 1e-15
        out[2 * i, G_COLUMN] = 2 * g[2 * i] / tot
        out[2 * i + 1, G_COLUMN] = 2 * g[2 * i + 1] / tot
    return out


def pitch_track(scores: np.ndarray, margin: Margin | None = None):
    """Outputs 18 and 19 (float64) and the tracked indices (F, 2) = (q_0, q_1) from the score rows of one trial."""
    S = len(scores)
    F = S // 2
    P = np.zeros(N_TRACK)
    p_all, best = 0.0, 0
    f18, f19, qs = np.zeros(F), np.zeros(F), np.zeros((F, 2), dtype=np.int64)
    qi = np.arange(N_TRACK)
    back = [None, None]
    for sf in range(S):
        xc, g = scores[sf, :N_TRACK], scores[sf, G_COLUMN]
        prev = np.full(N_TRACK, p_all - 6)
        ptr = np.full(N_TRACK, best)
        for k, d in enumerate(range(-4, 5)):
            ok = (qi + d >= 0) & (qi + d < N_TRACK)
            cand = np.where(ok, P[np.clip(qi + d, 0, N_TRACK - 1)] - _PEN[k], -np.inf)
            if margin is not None:
                margin.take((cand - prev)[ok])
            take = cand > prev
            prev = np.where(take, cand, prev)
            ptr = np.where(take, qi + d, ptr)
        Pn = prev + g * xc
        best = int(np.argmax(Pn))
        top = Pn[best]
        if margin is not None:
            margin.take(top - Pn)
        P = Pn - top
        p_all = top
        back[sf & 1] = ptr
        if sf & 1:
            i = sf // 2
            q1 = best
            q0 = int(back[1][q1])
            qs[i] = (q0, q1)
            period2 = min(max((256 - q0) + (256 - q1), 66), 510)
            f18[i] = 0.01 * (period2 - 200)
            f19[i] = (scores[sf - 1, G_COLUMN] * scores[sf - 1, q0] + g * scores[sf, q1]) / 2 - 0.5
    return f18, f19, qs


@dataclass
class Encoded:
    features: np.ndarray                  # float32 (F, 36)
    scores: np.ndarray                    # float64 (2 F, 256)
    lags: np.ndarray                      # int (F, 2): q_0, q_1
    cepstrum64: np.ndarray                # float64 (F, 18)
    margin: float = np.inf
    extra: dict = field(default_factory=dict)


def encode_trial(s: np.ndarray, lpc_fn, cepstrum32: np.ndarray | None = None, lpc: np.ndarray | None = None) -> Encoded:
    """One trial.  ``cepstrum32`` / ``lpc`` given: the residual, scores and track are computed from THOSE float32 values (how
    the GPU tests keep one-ulp cepstrum differences out of the scores); else from this statement's own."""
    s = np.asarray(s)
    F = len(s) // FRAME
    x = preemphasis(s)
    c64 = cepstrum(x, F)
    c32 = c64.astype(np.float32) if cepstrum32 is None else np.asarray(cepstrum32, dtype=np.float32)
    if lpc is None:
        lpc = np.stack([lpc_fn(c32[i]) for i in range(F)]) if F else np.zeros((0, LPC_ORDER), np.float32)
    lpc = np.asarray(lpc, dtype=np.float32).reshape(F, LPC_ORDER)
    m = Margin()
    sc = subframe_scores(residual(x, lpc, F), F, m)
    f18, f19, qs = pitch_track(sc, m)
    feats = np.zeros((F, N_OUT), np.float32)
    feats[:, :NB_BANDS] = c32
    feats[:, 18] = f18
    feats[:, 19] = f19
    feats[:, 20:] = lpc
    return Encoded(feats, sc, qs, c64, m.value)


def encode_trials(audio: np.ndarray, offsets, lpc_fn, cepstrum32=None, lpc=None):
    """A trial list over a concatenation: ([Encoded per trial], frame_offsets)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    fo = np.concatenate([[0], np.cumsum((offsets[1:] - offsets[:-1]) // FRAME)]).astype(np.int64)
    out = []
    for i in range(len(offsets) - 1):
        a, b = fo[i], fo[i + 1]
        out.append(encode_trial(audio[offsets[i]:offsets[i + 1]], lpc_fn,
                                None if cepstrum32 is None else cepstrum32[a:b], None if lpc is None else lpc[a:b]))
    return out, fo
