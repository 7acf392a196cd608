"""The corpus and the case table of the trial-list validation tests (tests/test_cpu_validation.py, tests/test_gpu_validation.py): a
helper module like lstm_reference.py, no tests in it.

The corpus: one (N_ROWS, 64) array of N(0, 1) x 2 frames per weight scale and a trial list over it with lengths 1, 3, 4, 5, 50, 251
and 1500 (chunk tails of every size, one frame, a whole long trial), overlapping ranges, out of order.  It pins the path at the
reference's sizes (H = 150 / 100, C = 64, 20 outputs) on decoder handles of 3, 4, 5 and 64 streams, where every chunk runs one
trial per workgroup.

The case table names the smallest runs that reach the rest of what Part 8 does:

  DECODER   ``dss_launch_decoder_trials`` picks the streams per workgroup W from the chunk's trial count (1 up to
            ``WIDTH_1_UP_TO`` = 128 trials, 2 up to ``WIDTH_2_UP_TO`` = 256, 4 beyond).  At W = 2 / 4 the workgroup partners come from
            the longest-first order, ``in_row`` is a frame index (one frame per "row"), and ``dec_regress_trials_kernel`` scatters
            the padded (trials x longest) grid to ``out_row[...]`` in blocks of ``REGRESS_ROWS`` = 8 rows:
              width        300 trials of 1 .. 9 frames at (7, 5) on handles of 300 (one W = 4 chunk), 256 (a W = 2 chunk, then a
                           W = 1 chunk of 44) and 129 streams (two W = 2 chunks, then a W = 1 chunk of 42)
              mixed        140 trials, lengths 17, 16, 9, 8, 1 once each and the rest 1 .. 7: one W = 2 chunk whose longest trial
                           is no multiple of 8, blocks of pure padding (the early return) beside blocks that straddle a trial's end
              reference    130 trials of 1 .. 12 frames at (100, 64) through ``decoder_validation(state_dict, ...)`` with
                           ``max_streams`` left alone: the W = 2 chunk a real corpus of more than 128 trials starts with
              odd sizes    (33, 17) with 1 output, (127, 255) with 31 (K = 2H = 254 = 2 modulo 4), (128, 256) with 32 (the largest K
                           and the largest dynamic LDS, O (2H + 1) + 8 x 2H floats), (1, 1) with 3; trials of 1, 3, 4, 5, 8, 9
                           frames on a handle of 2 streams
  DETECTOR  ``vad_trials_kernel`` is a compile of its own of the forward body (5 waves per SIMD asked for): (7, 5), (33, 17) and
            (159, 127) -- ``Hp`` / ``Cp`` padding --, the capacity corner (160, 128) with a trial of 257 frames, (1, 1); and TIE, a
            (7, 5) detector whose two classifier rows are equal, so every logit pair is equal bit for bit
  score     synthetic logits handed straight to ``dss_vad_score_trials_dev``: trials of 1, 255, 256, 257, 512, 513 frames (the
            256-frame tile), N(0, 3) logits mixed with runs of (+800, -800) and (-800, +800), where exp(z - m) underflows to 0 in
            float64, and runs of equal logits
  MSE       (frames, outputs) on either side of ``dec_mse_trials_kernel``'s stride of 256 elements

Every entry's frames are N(0, 1) x 2 (``lstm_reference.frames``), its trials lie side by side in an array of its own without
overlap -- so no two trials hold the same frames -- in an order that is neither the list's nor longest-first.  The detector
entries' seeds are chosen so that the float64 detector has no near-tie on any frame, like ``SEEDS``;
tests/test_cpu_validation.py asserts every condition stated here on the float64 reference alone."""
import collections
import functools
import os
import re

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


# ---- the case table ---------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "delayed-speech-synthesis_amd", "csrc")

WIDTH_1_UP_TO, WIDTH_2_UP_TO = 128, 256          # trials of a chunk up to which a workgroup holds 1 / 2 of them (4 beyond)
REGRESS_ROWS = 8                                 # DEC_RROWS: rows of the padded grid per block of dec_regress_trials_kernel
TRIAL_CHUNK = 256                                # DSS_TRIAL_CHUNK: trials per launch of the two reduction kernels
SCORE_TILE = 256                                 # SCORE_THREADS: frames per tile of vad_score_trials_kernel
MSE_STRIDE = 256                                 # elements per pass of dec_mse_trials_kernel


def source_constants():
    """The constants above as the sources state them (tests/test_cpu_validation.py compares)."""
    def text(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def define(src, name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))
    dec, vad, common, blocks = text("bilstm_decoder.hip"), text("vad_lstm.hip"), text("dss_common.h"), text("lstm_blocks.h")
    # both decoder launchers take the streams per workgroup from dss_dec_streams_per_wg
    assert len(re.findall(r"const int W = dss_dec_streams_per_wg\(S\);", dec)) == 1 and "Wsel" not in dec
    w = re.search(r"int dss_dec_streams_per_wg\(int S\) \{ return 2 \* S <= (\d+) \? 1 : \(S <= (\d+) \? 2 : 4\); \}", common)
    mse = dec[dec.index("dec_mse_trials_kernel(DssTrialLens"):]
    return dict(WIDTH_1_UP_TO=int(w.group(1)) // 2, WIDTH_2_UP_TO=int(w.group(2)), REGRESS_ROWS=define(blocks, "DEC_RROWS"),
                TRIAL_CHUNK=define(common, "DSS_TRIAL_CHUNK"), SCORE_TILE=define(vad, "SCORE_THREADS"),
                MSE_STRIDE=int(re.search(r"i < n; i \+= (\d+)\)", mse).group(1)), DEC_MAXO=define(common, "DSS_DEC_MAXO"),
                VAD_MAX=(define(common, "DSS_VAD_MAXH"), define(common, "DSS_VAD_MAXC")),
                DEC_MAX=(define(common, "DSS_DEC_MAXH"), define(common, "DSS_DEC_MAXC")))


def longest_first(lengths):
    """``trials_longest_first`` (csrc/dss_host.cpp): list positions, longest trial first, ties in list order."""
    return sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))


def decoder_chunks(lengths, handle_streams):
    """[(trials, longest, W)] of the chunks ``dss_dec_forward_trials_dev`` cuts a list into on a handle of that many streams."""
    order = longest_first(lengths)
    out = []
    for k0 in range(0, len(order), handle_streams):
        s = min(handle_streams, len(order) - k0)
        out.append((s, lengths[order[k0]], 1 if s <= WIDTH_1_UP_TO else 2 if s <= WIDTH_2_UP_TO else 4))
    return out


def regress_blocks(lengths_sorted):
    """(blocks of pure padding, blocks that hold a trial's last row and a padded row behind it, blocks) of one chunk's padded grid."""
    T = lengths_sorted[0]
    live = (np.arange(T)[None, :] < np.asarray(lengths_sorted)[:, None]).ravel()
    live = np.concatenate([live, np.zeros(-len(live) % REGRESS_ROWS, bool)]).reshape(-1, REGRESS_ROWS)
    straddle = (live[:, :-1] & ~live[:, 1:]).any(axis=1)
    return int((~live.any(axis=1)).sum()), int(straddle.sum()), len(live)


def _layout(lengths, seed, in_list_order=False):
    """[(first, len)] in list order and the rows they take: the trials side by side without overlap, in a shuffled order (or the
    list's: a corpus as ``decoder_validation`` takes it)."""
    n = len(lengths)
    place = np.arange(n) if in_list_order else np.random.default_rng(seed).permutation(n)
    first, row = [0] * n, 0
    for i in place:
        first[i] = row
        row += lengths[i]
    return [(int(first[i]), int(lengths[i])) for i in range(n)], row


def _random_lengths(seed, n, longest, fixed=()):
    """`fixed` and n - len(fixed) lengths of 1 .. longest, shuffled."""
    rng = np.random.default_rng(seed)
    v = np.concatenate([np.asarray(fixed, np.int64), rng.integers(1, longest + 1, n - len(fixed))])
    return tuple(int(a) for a in rng.permutation(v))


DecEntry = collections.namedtuple("DecEntry", "name H C O scale handles lengths corpus_form")
VadEntry = collections.namedtuple("VadEntry", "H C scale lengths seed")

ODD_LENGTHS = (1, 3, 4, 5, 8, 9)
DECODER = (
    # ---- streams per workgroup
    DecEntry("width", 7, 5, 20, 1, (300, 256, 129), _random_lengths(41, 300, 9), False),
    DecEntry("mixed", 7, 5, 20, 1, (256,), _random_lengths(42, 140, 7, fixed=(17, 16, 9, 8, 1)), False),
    DecEntry("reference", 100, 64, 20, 1, (None,), _random_lengths(43, 130, 12), True),          # None: decoder_validation's own handle
    # ---- odd sizes and output counts
    DecEntry("odd", 33, 17, 1, 1, (2,), ODD_LENGTHS, False),
    DecEntry("odd", 33, 17, 1, 4, (2,), ODD_LENGTHS, False),
    DecEntry("odd", 127, 255, 31, 1, (2,), ODD_LENGTHS, False),
    DecEntry("odd", 128, 256, 32, 1, (2,), ODD_LENGTHS, False),
    DecEntry("odd", 1, 1, 3, 1, (2,), ODD_LENGTHS, False),
)
WIDTH, MIXED, REFERENCE_SIZE = DECODER[0], DECODER[1], DECODER[2]
DECODER_VALIDATION = DECODER[4]                  # (33, 17), 1 output, x4: decoder_validation's sums on an odd size
F64_FRAMES_UP_TO = 17                            # entries whose trials have at most this many frames also run with float64 frames

# seed: the first of 9400 + 50 i (i the entry's position), 9401 + 50 i, ... at which the float64 detector has no near-tie
DETECTOR = (
    VadEntry(7, 5, 1, (1, 3, 4, 5, 9), 9400),
    VadEntry(7, 5, 4, (1, 3, 4, 5, 9), 9450),
    VadEntry(33, 17, 1, (1, 3, 4, 5, 9), 9500),
    VadEntry(33, 17, 4, (1, 3, 4, 5, 9), 9550),
    VadEntry(159, 127, 1, (1, 3, 4, 5, 9), 9600),
    VadEntry(160, 128, 1, (1, 4, 5, 257), 9650),
    VadEntry(160, 128, 4, (1, 4, 5, 257), 9700),
    VadEntry(1, 1, 1, (1, 5), 9750),
)
TIE = VadEntry(7, 5, 1, (1, 3, 4, 5, 9), 9800)   # runs on tie_state_dict(): every logit pair equal
DETECTOR_VALIDATION = DETECTOR[3]                # (33, 17) x4: vad_validation's sums on an odd size

SCORE_LENGTHS = (1, 255, 256, 257, 512, 513)
UNDERFLOW = 800.0                                # exp(-1600) = 0 in float64
MSE_CASES = ((255, 1), (256, 1), (257, 1), (8, 32), (9, 31), (1, 1), (86, 3))          # (frames, outputs)


def dec_ident(e: DecEntry) -> str:
    return f"{e.name}-{e.H}-{e.C}-{e.O}-x{e.scale}"


def vad_ident(e: VadEntry) -> str:
    return f"{e.H}-{e.C}-x{e.scale}"


def bounds_of(lengths):
    b = np.concatenate([[0], np.cumsum(lengths)])
    return [slice(int(b[k]), int(b[k + 1])) for k in range(len(lengths))]


def decoder_state_dict(H: int, C: int, scale: int, O: int):
    """``lstm_reference.decoder_state_dict`` with a regressor of O outputs (20: its own; otherwise ``nn.Linear(2H, O)`` at
    torch's default init from a seed of the size's)."""
    sd = R.decoder_state_dict(H, C, scale)
    if O != 20:
        import torch
        torch.manual_seed(400 + 7 * H + O)
        head = torch.nn.Linear(2 * H, O)
        sd["regressor.weight"], sd["regressor.bias"] = head.weight.detach().clone(), head.bias.detach().clone()
    return sd


def tie_state_dict():
    """The (7, 5) detector with classifier row 1 made a copy of row 0, bias included."""
    sd = R.vad_state_dict(TIE.H, TIE.C, TIE.scale)
    w, b = sd["classifier.weight"].clone(), sd["classifier.bias"].clone()
    w[1], b[1] = w[0], b[0]
    sd["classifier.weight"], sd["classifier.bias"] = w, b
    return sd


@functools.lru_cache(maxsize=None)
def decoder_inputs(e: DecEntry):
    """state_dict, frames (N, C) float64 holding float32 values, [(first, len)] of a decoder entry.  Shared: not to be written to."""
    i = DECODER.index(e)
    ranges, n = _layout(e.lengths, 9200 + i, in_list_order=e.corpus_form)
    return decoder_state_dict(e.H, e.C, e.scale, e.O), R.frames("x2", 1, n, e.C, 9250 + i)[0], ranges


def _pool(x, ranges):
    pool = np.zeros((len(ranges), max(n for _, n in ranges), x.shape[1]))
    for i, (a, n) in enumerate(ranges):
        pool[i, :n] = x[a:a + n]
    return pool


@functools.lru_cache(maxsize=None)
def decoder_truth(e: DecEntry):
    """The float64 decoder on every trial of the entry: (trials, longest, O), zero beyond a trial's length.  Computed once."""
    sd, x, ranges = decoder_inputs(e)
    return R.decoder_forward(R.Net(sd), _pool(x, ranges), lengths=[n for _, n in ranges])[0]


def decoder_top(model, pool, lengths):
    """The float64 decoder in front of its regressor: (trials, longest, 2H), zero beyond a trial's length."""
    net = R.as_net(model)
    inp = np.asarray(pool, np.float64)
    for layer in (0, 1):
        inp = np.concatenate([R.lstm_layer(net, layer, inp, lengths=lengths)[0],
                              R.lstm_layer(net, layer, inp, reverse=True, lengths=lengths)[0]], axis=2)
    return inp


def regress_trials(top, w, b, lengths, handle_streams, defect=None):
    """``dec_regress_trials_kernel`` over the chunks of ``dss_dec_forward_trials_dev`` in numpy float64: `top` (trials, longest,
    2H) in LIST order -> (sum len, O) in list order.  defect "out_row_in_list_order": chunk position k writes to where list
    position k starts, not to where the trial it holds starts; "first_padded_row_live": the row behind a trial's last one counts as
    live where the chunk's grid has one (the layers leave zeros there), and what it writes stays."""
    assert defect in (None, "out_row_in_list_order", "first_padded_row_live")
    lengths = [int(n) for n in lengths]
    start = np.concatenate([[0], np.cumsum(lengths)])
    order = longest_first(lengths)
    out = np.full((int(start[-1]) + 1, w.shape[0]), np.nan)          # (one spare row: the last trial's padded row lands there)
    late = []
    for k0 in range(0, len(order), handle_streams):
        chunk = order[k0:k0 + handle_streams]
        T = lengths[chunk[0]]
        for k, i in enumerate(chunk, start=k0):
            row = int(start[k if defect == "out_row_in_list_order" else i])
            out[row:row + lengths[i]] = top[i, :lengths[i]] @ w.T + b
            if defect == "first_padded_row_live" and lengths[i] < T:
                late.append((row + lengths[i], np.zeros(top.shape[2]) @ w.T + b))
    for row, v in late:
        out[row] = v
    return out[:-1]


@functools.lru_cache(maxsize=None)
def detector_inputs(e: VadEntry):
    """state_dict, frames (N, C) float64 holding float32 values, [(first, len)] of a detector entry.  Shared: not to be written to."""
    ranges, n = _layout(e.lengths, e.seed + 7000)
    return (tie_state_dict() if e == TIE else R.vad_state_dict(e.H, e.C, e.scale)), R.frames("x2", 1, n, e.C, e.seed)[0], ranges


@functools.lru_cache(maxsize=None)
def detector_truth(e: VadEntry):
    """The float64 detector on every trial from the zero state: (sum len, 2) in list order.  Computed once."""
    sd, x, ranges = detector_inputs(e)
    net = R.Net(sd)
    return np.concatenate([R.vad_forward(net, x[None, a:a + n])[0][0] for a, n in ranges])


FRAME_KINDS = ("random", "first wins by the whole gap", "second wins by the whole gap", "equal")


@functools.lru_cache(maxsize=None)
def score_inputs():
    """Synthetic inputs of ``dss_vad_score_trials_dev``: float32 logits (sum SCORE_LENGTHS, 2), the kind of every frame (an index
    into FRAME_KINDS; runs of 11 frames), the strict argmax as int32 labels, and uint8 targets in runs of 7 frames, so that every
    run of a kind meets both targets."""
    n = sum(SCORE_LENGTHS)
    rng = np.random.default_rng(9301)
    z = (rng.standard_normal((n, 2)) * 3.0).astype(np.float32)
    kind = np.repeat(np.resize((0, 1, 0, 2, 3, 0, 0, 2, 1, 3), n // 11 + 1), 11)[:n]
    z[kind == 1] = (UNDERFLOW, -UNDERFLOW)
    z[kind == 2] = (-UNDERFLOW, UNDERFLOW)
    z[kind == 3, 1] = z[kind == 3, 0]
    argmax = (z[:, 1] > z[:, 0]).astype(np.int32)
    runs = np.repeat(np.resize((0, 1), n // 7 + 1), 7)[:n].astype(np.uint8)
    return z, kind, argmax, runs


def softmax_speech(logits):
    """softmax(z)[1] per frame in float64, as exp(z1 - logsumexp(z))."""
    z = np.asarray(logits, np.float64)
    m = z.max(axis=1)
    return np.exp(z[:, 1] - (m + np.log(np.exp(z[:, 0] - m) + np.exp(z[:, 1] - m))))


def mse_inputs(frames: int, outputs: int):
    """A trial of `frames` frames between one of 3 and one of 2: lengths, float32 features and targets (sum len, outputs)."""
    rng = np.random.default_rng(9500 + 40 * frames + outputs)
    lengths = (3, frames, 2)
    return lengths, rng.standard_normal((sum(lengths), outputs)).astype(np.float32), rng.standard_normal((sum(lengths), outputs)).astype(np.float32)
