"""float64 numpy statement of the acoustic contamination analysis (dss_amd/contamination.py, Part 12 of include/dss_hip.h), and the
error bounds the GPU tests hold the kernels to.  The MATLAB toolbox the reference drives is not part of it, so THIS is the
definition (DESIGN.md restates it); parity with the toolbox is not pinned.

Definition.  brain (T, C), audio (T,), one rate.  Frames of nperseg rows every hop rows, no padding, W = (T - nperseg) // hop + 1;
per frame the rows times the symmetric Hamming window, a direct DFT of length nperseg, the magnitude at the kept bins; no
detrending, no scale (no correlation sees one).  Frame t is kept iff all its samples are.  For lag l in -L .. L the pairs are
the frames t with 0 <= t + l < W, keep[t] and keep[t + l]; r[l, c, i, j] is the Pearson correlation of audio bin i at t + l with
bin j of channel c at t over the pairs, two-pass (means first); NaN with fewer than two pairs or zero variance on either side,
where a variance counts as zero when sum (x - mean)^2 <= 4 n 2^-53 sum x^2.

Bounds (derived, not measured; U = 2^-53, n = nperseg, P = pairs of a lag).  The DFT sums are n-term sums of products of
rounded factors: |d re|, |d im| <= (n + 8) U sum_k |x_k w_k| on either side (the 8: window, table, square root and magnitude
roundings), so a magnitude computed twice differs by at most e[t] = 2 (n + 8) U sum_k |x_k w_k|; the audio's also carries the
rounding of the subtraction, U (|a| + |shift|).  A P-term sum of products of such values, added in any order with fused or
plain multiply-adds, then differs by at most the terms' own differences plus (P + 8) U sum |term|:
    d sb  = sum eb + (P + 8) U sum b               d sbb = sum (2 b eb + eb^2) + (P + 8) U sum b^2
    d sab = sum (|a| eb + b ea + ea eb) + (P + 8) U sum |a| b           (and d sa, d saa like d sb, d sbb).
To first order, with cov = sab - sa sb / P, va = saa - sa^2 / P, vb = sbb - sb^2 / P:
    d cov = d sab + (|sa| d sb + |sb| d sa) / P + 4 U (|sab| + |sa sb| / P)
    d va  = d saa + 2 |sa| d sa / P + 4 U (saa + sa^2 / P)              (d vb alike)
    d r   = d cov / sqrt(va vb) + |r| (d va / va + d vb / vb) / 2 + 4 U |r|.
"""
import numpy as np

U = 2.0 ** -53


def hamming(n):
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))


def frames_of(T, nperseg, hop):
    return (T - nperseg) // hop + 1


def kept_bins(fs, nperseg, band):
    f = np.arange(nperseg // 2 + 1) * fs / nperseg
    return np.where((f >= band[0]) & (f <= band[1]))[0]


def spectrogram(x, window, nperseg, hop, bins):
    """x (T, C) -> (magnitudes (W, C, len(bins)), sum_k |x_k w_k| (W, C))."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    W = frames_of(len(x), nperseg, hop)
    seg = x[np.arange(W)[:, None] * hop + np.arange(nperseg)[None, :]] * np.asarray(window)[None, :, None]      # (W, nperseg, C)
    ang = 2.0 * np.pi * ((np.asarray(bins)[:, None] * np.arange(nperseg)[None, :]) % nperseg) / nperseg
    re = np.einsum("bn,wnc->wcb", np.cos(ang), seg)
    im = np.einsum("bn,wnc->wcb", np.sin(ang), seg)
    return np.sqrt(re * re + im * im), np.abs(seg).sum(axis=1)


def frame_mask(keep, nperseg, hop):
    W = frames_of(len(keep), nperseg, hop)
    return np.array([bool(np.all(keep[t * hop:t * hop + nperseg])) for t in range(W)])


def pairs(W, lag, fm):
    """The frames t of a lag's pairs."""
    t = np.arange(max(0, -lag), min(W, W - lag))
    if len(t) == 0:
        return t
    return t[fm[t] & fm[t + lag]]


def zero_variance(x):
    """Over the last axis: sum (x - mean)^2 <= 4 n U sum x^2."""
    n = x.shape[-1]
    v = np.sum((x - x.mean(axis=-1, keepdims=True)) ** 2, axis=-1)
    return v <= 4 * n * U * np.sum(x * x, axis=-1)


class Day:
    """The spectrograms of one recording, computed once."""

    def __init__(self, brain, audio, fs, window=0.2, spg_fs=50, band=(70, 170), max_lag=0.5, keep=None):
        self.nperseg, self.hop, self.L = int(round(window * fs)), int(round(fs / spg_fs)), int(round(max_lag * spg_fs))
        self.bins = kept_bins(fs, self.nperseg, band)
        w = hamming(self.nperseg)
        self.N, self.absN = spectrogram(brain, w, self.nperseg, self.hop, self.bins)          # (W, C, B), (W, C)
        A, absA = spectrogram(audio, w, self.nperseg, self.hop, self.bins)
        self.A, self.absA = A[:, 0], absA[:, 0]                                               # (W, B), (W,)
        self.W = len(self.A)
        self.fm = np.ones(self.W, dtype=bool) if keep is None else frame_mask(np.asarray(keep, dtype=bool), self.nperseg, self.hop)

    def correlations(self):
        """(2 L + 1, C, B, B) two-pass Pearson correlations, NaN where undefined."""
        C, B = self.N.shape[1], len(self.bins)
        r = np.full((2 * self.L + 1, C, B, B), np.nan)
        for li, lag in enumerate(range(-self.L, self.L + 1)):
            t = pairs(self.W, lag, self.fm)
            if len(t) < 2:
                continue
            a, b = self.A[t + lag].T, self.N[t].transpose(1, 2, 0)                            # (B, P), (C, B, P)
            za, zb = zero_variance(a), zero_variance(b)
            a = a - a.mean(axis=-1, keepdims=True)
            b = b - b.mean(axis=-1, keepdims=True)
            with np.errstate(divide="ignore", invalid="ignore"):
                v = np.einsum("ip,cjp->cij", a, b) / np.sqrt(np.sum(a * a, axis=-1)[None, :, None] * np.sum(b * b, axis=-1)[:, None, :])
            v[:, za, :] = np.nan
            v[zb[:, None, :] & np.ones((1, B, 1), dtype=bool)] = np.nan
            r[li] = v
        return r

    def moments(self, shift):
        """The six sums with the audio less `shift` (B,), and their bounds: two dicts of n, sa, saa, sb, sbb, sab."""
        C, B, n = self.N.shape[1], len(self.bins), self.nperseg
        nl = 2 * self.L + 1
        m = {"n": np.zeros(nl), "sa": np.zeros((nl, B)), "saa": np.zeros((nl, B)), "sb": np.zeros((nl, C, B)), "sbb": np.zeros((nl, C, B)),
             "sab": np.zeros((nl, C, B, B))}
        d = {k: np.zeros_like(v) for k, v in m.items()}
        A = self.A - shift[None, :]
        eA = 2 * (n + 8) * U * self.absA[:, None] + U * (np.abs(self.A) + np.abs(shift)[None, :])        # (W, B)
        eN = np.broadcast_to(2 * (n + 8) * U * self.absN[:, :, None], self.N.shape)                      # (W, C, B)
        for li, lag in enumerate(range(-self.L, self.L + 1)):
            t = pairs(self.W, lag, self.fm)
            P = len(t)
            m["n"][li] = P
            if P == 0:
                continue
            a, ea, b, eb = A[t + lag], eA[t + lag], self.N[t], eN[t]
            g = (P + 8) * U
            m["sa"][li] = a.sum(0)
            d["sa"][li] = ea.sum(0) + g * np.abs(a).sum(0)
            m["saa"][li] = (a * a).sum(0)
            d["saa"][li] = (2 * np.abs(a) * ea + ea * ea).sum(0) + g * (a * a).sum(0)
            m["sb"][li] = b.sum(0)
            d["sb"][li] = eb.sum(0) + g * b.sum(0)
            m["sbb"][li] = (b * b).sum(0)
            d["sbb"][li] = (2 * b * eb + eb * eb).sum(0) + g * (b * b).sum(0)
            m["sab"][li] = np.einsum("pi,pcj->cij", a, b)
            d["sab"][li] = (np.einsum("pi,pcj->cij", np.abs(a), eb) + np.einsum("pi,pcj->cij", ea, b) + np.einsum("pi,pcj->cij", ea, eb)
                            + g * np.einsum("pi,pcj->cij", np.abs(a), b))
        return m, d


def r_bound(m, d):
    """The first-order bound on r from the sums and their bounds (dicts of Day.moments); inf where r is undefined."""
    with np.errstate(divide="ignore", invalid="ignore"):
        P = m["n"][:, None, None, None]
        sa, dsa = m["sa"][:, None, :, None], d["sa"][:, None, :, None]
        saa, dsaa = m["saa"][:, None, :, None], d["saa"][:, None, :, None]
        sb, dsb = m["sb"][:, :, None, :], d["sb"][:, :, None, :]
        sbb, dsbb = m["sbb"][:, :, None, :], d["sbb"][:, :, None, :]
        sab, dsab = m["sab"], d["sab"]
        cov, va, vb = sab - sa * sb / P, saa - sa * sa / P, sbb - sb * sb / P
        dcov = dsab + (np.abs(sa) * dsb + np.abs(sb) * dsa) / P + 4 * U * (np.abs(sab) + np.abs(sa * sb) / P)
        dva = dsaa + 2 * np.abs(sa) * dsa / P + 4 * U * (saa + sa * sa / P)
        dvb = dsbb + 2 * np.abs(sb) * dsb / P + 4 * U * (sbb + sb * sb / P)
        r = cov / np.sqrt(va * vb)
        out = dcov / np.sqrt(va * vb) + np.abs(r) * (dva / va + dvb / vb) / 2 + 4 * U * np.abs(r)
    out[~np.isfinite(out)] = np.inf
    return out


def contamination_matrix(r0):
    out = np.full(r0.shape[1:], np.nan)
    for i in range(r0.shape[1]):
        for j in range(r0.shape[2]):
            v = r0[:, i, j]
            v = v[~np.isnan(v)]
            if len(v):
                out[i, j] = v.max()
    return out


def criterion(M, n_surrogates=10000, seed=0):
    """(surrogates (S,), dataset measure, P): column permutations from numpy.random.Generator(PCG64(seed)).  With a NaN on the
    diagonal the measure is NaN and so is P: nothing was compared."""
    rng = np.random.Generator(np.random.PCG64(seed))
    B = len(M)
    sur = np.array([np.mean([M[i, p[i]] for i in range(B)]) for p in (rng.permutation(B) for _ in range(n_surrogates))])
    measure = np.mean(np.diag(M))
    return sur, measure, (np.nan if np.isnan(measure) else np.count_nonzero(sur >= measure) / n_surrogates)


# ---- the planted case both test files run ----------------------------------------------------------------------------
PLANT_SEED, PLANT_FS, PLANT_T, PLANT_C, PLANT_CHANNEL, PLANT_AUDIO_GAIN = 11, 1000, 20000, 12, 5, 4.0


def planted_case(plant):
    """Seeded unit-variance noise channels and noise audio of standard deviation 4; with `plant`, channel 5 also carries
    0.3 x the audio.  20 s at 1 kHz: 991 frames."""
    rng = np.random.default_rng(PLANT_SEED)
    brain = rng.standard_normal((PLANT_T, PLANT_C))
    audio = PLANT_AUDIO_GAIN * rng.standard_normal(PLANT_T)
    if plant:
        brain[:, PLANT_CHANNEL] += 0.3 * audio
    return brain, audio
