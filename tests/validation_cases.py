"""The corpus of the trial-list validation tests (tests/test_cpu_validation.py, tests/test_gpu_validation.py): a helper module
like lstm_reference.py.  One (N_ROWS, 64) array of N(0, 1) x 2 frames per weight scale and a trial list over it with lengths
1, 3, 4, 5, 50, 251 and 1500 (chunk tails of every size, one frame, a whole long trial), overlapping ranges, out of order."""
import numpy as np

import lstm_reference as R

VAD_H, DEC_H, C = 150, 100, 64
N_ROWS = 2000
# (first, len): the long trial overlaps four others, two trials are the same rows, the last row of the array is used
RANGES = [(300, 50), (0, 1500), (1490, 5), (7, 1), (100, 251), (1700, 4), (1702, 3), (100, 251), (1999, 1), (1200, 251)]
# the frames' seeds per weight scale.  Chosen so that the float64 detector has no near-tie on any frame of any trial:
# |z1 - z0| > 2 x lstm_reference.bound(scale) everywhere (tests/test_cpu_validation.py asserts it), so a kernel within the bound
# must give the float64 labels on every frame.
SEEDS = {1: 9101, 4: 9104}


def corpus(scale: int):
    """(N_ROWS, C) float64 frames holding float32 values."""
    return R.frames("x2", 1, N_ROWS, C, SEEDS[scale])[0]


def targets(scale: int):
    """uint8 (sum len,) 0 / 1 targets in concatenated trial order: runs of speech and silence, as acoustic labels come."""
    rng = np.random.default_rng(SEEDS[scale] + 1)
    n = sum(length for _, length in RANGES)
    return np.repeat(rng.integers(0, 2, n // 20 + 1), 20)[:n].astype(np.uint8)


def lpc_targets(scale: int, n_outputs: int = 20):
    """float32 (sum len, n_outputs) regression targets in concatenated trial order."""
    rng = np.random.default_rng(SEEDS[scale] + 2)
    return rng.standard_normal((sum(length for _, length in RANGES), n_outputs)).astype(np.float32)


def vad_reference_logits(scale: int):
    """The float64 detector on every trial from the zero state: (sum len, 2) in concatenated trial order."""
    net = R.Net(R.vad_state_dict(VAD_H, C, scale))
    x = corpus(scale)
    return np.concatenate([R.vad_forward(net, x[None, a:a + n])[0][0] for a, n in RANGES])


def cross_entropy(logits, target):
    """Per frame logsumexp(z) - z[target] in float64 (nn.CrossEntropyLoss before its mean)."""
    z = np.asarray(logits, np.float64)
    m = z.max(axis=1)
    lse = m + np.log(np.exp(z[:, 0] - m) + np.exp(z[:, 1] - m))
    return lse - z[np.arange(len(z)), np.asarray(target, np.int64)]


def trial_slices():
    b = np.concatenate([[0], np.cumsum([n for _, n in RANGES])])
    return [slice(int(b[k]), int(b[k + 1])) for k in range(len(RANGES))]
