"""Cases of the two BPTT trainers (csrc/dec_train.hip, csrc/vad_train.hip) for the tests (helper module, no tests in it).

``GRAD_CASES`` of decoder_training_reference.py and vad_training_reference.py sit at the reference architecture and two neighbours:
every hidden size is a multiple of 2, no detector window is longer than 50 frames, no decoder trial longer than 350, and the
decoder's gradients are pinned at 20 outputs only.  ``DECODER`` and ``DETECTOR`` name the smallest runs that reach the rest of
what the kernels do:

  odd sizes   H = 1, 3 modulo 4 and odd C: the ``Hp`` / ``Cp`` padding of the packed copies, ``if (4 * k >= H) break`` with its
              four-wide loads of ``dgs`` in ``dec_train_bptt_body``, the remainder loops of ``vad_tdot`` (8-wide) and of the
              W_ih_l1 pass (4-wide), the packed-copy index ``ki = Cp + (k - nA)`` of both step kernels; the decoder's layer 1 then
              has 2H = 2 modulo 4 inputs.  (127, 255) and (159, 127) are the largest odd sizes the kernels take
  smallest    H = C = 1
  tiles       the 8-frame tiles of the decoder's head (``DEC_RROWS``) and dmid (``DTM_FR``) kernels at T = 8, 16 and 17: one full
              tile, two, and two with one frame behind them (the ``tt < nst`` zero fill)
  long        the 256-frame tile of both step kernels (``DTS_THREADS``, ``VTS_THREADS``) at its edge, T = 256 and 257; the second
              pass of ``dec_train_loss_body``'s stride of ``DEC_THREADS`` = 512 (T = 513) and the third (1025); the second pass
              of the detector's loss / dlogits loop, a stride of ``VAD_THREADS`` = 640 (T = 641)
  outputs     O = 1 and ``DSS_DEC_MAXO`` = 32, which size the head's dynamic LDS and the step kernel's grid (16 H + O), and
              3, 4, 31 beside the 20 of every other test

An entry is (H, C, T, scale of the LSTM weights, O or None for the detector, the masks it runs with).  Its inputs are those of the
helper modules' ``case_inputs`` (N(0, 1) x 2 frames that hold float32 values, mask multipliers of 0 / 2, seeded from the case);
the decoder's regressor is drawn for the entry's output count.  A detector's trainer is created with ``max_window`` = T.

Every entry runs without a mask and with a random one, but H = 1: there a random mask can zero the whole true gradient of a tensor,
and an error relative to zero says nothing, so H = 1 runs without a mask and with a mask of all 2.0 ("twos").

The bound of the GPU tests is the helper modules' ``GRAD_BOUND``, 4 x the error of torch float32 CPU autograd against float64; the
table holds only inputs on which torch float32 alone stays within ``GRAD_BOUND / 4`` (tests/test_cpu_training_cases.py asserts
it per entry and mask; tools/decoder_training_bounds.py and tools/vad_training_bounds.py print the figures).  Long cases have
H = 6 or 16, so that their float64 autograd takes about a second; the detector's (150, 64, 257) is the one exception: the
256-frame tile at the reference width, where both columns of a thread of the step kernel are live."""
from __future__ import annotations

import collections
import functools

import numpy as np

import decoder_training_reference as D
import vad_training_reference as V

DEC_THREADS = 512                # the stride of dec_train_loss_body
VAD_THREADS = 640                # the stride of the detector's loss / dlogits loop
STEP_TILE = 256                  # DTS_THREADS, VTS_THREADS: frames per pass of the step kernels' sum over t
FRAME_TILE = 8                   # DEC_RROWS, DTM_FR: frames per workgroup of the decoder's head and dmid kernels
DEC_MAXO = 32                    # DSS_DEC_MAXO

Entry = collections.namedtuple("Entry", "H C T scale O masks")

BOTH = (None, "random")
ONE_UNIT = (None, "twos")

DECODER = (
    # ---- odd sizes
    Entry(7, 5, 9, 1, 20, BOTH),
    Entry(7, 5, 9, 4, 20, BOTH),
    Entry(33, 17, 17, 1, 20, BOTH),
    Entry(127, 255, 5, 1, 31, BOTH),
    # ---- the smallest legal size
    Entry(1, 1, 3, 1, 20, ONE_UNIT),
    # ---- frame tiles and output counts
    Entry(6, 5, 8, 1, 1, BOTH),
    Entry(6, 5, 16, 1, 32, BOTH),
    Entry(6, 5, 17, 1, 3, BOTH),
    Entry(6, 5, 256, 1, 20, BOTH),
    Entry(6, 5, 257, 1, 20, BOTH),
    Entry(6, 5, 513, 1, 20, BOTH),
    Entry(16, 8, 1025, 1, 4, BOTH),
)

DETECTOR = (
    # ---- odd sizes
    Entry(7, 5, 9, 1, None, BOTH),
    Entry(33, 17, 17, 1, None, BOTH),
    Entry(159, 127, 5, 1, None, BOTH),
    # ---- the smallest legal size
    Entry(1, 1, 3, 1, None, ONE_UNIT),
    # ---- long windows
    Entry(6, 5, 256, 1, None, BOTH),
    Entry(6, 5, 257, 1, None, BOTH),
    Entry(6, 5, 641, 1, None, BOTH),
    Entry(150, 64, 257, 1, None, BOTH),
)

F64_FRAMES_UP_TO = 17            # entries of at most this many frames also run with float64 frames

# where the trainers are held to float64 again after update steps, and where the RMSprop formula is checked
DECODER_AFTER_STEPS = (DECODER[0], DECODER[2], DECODER[7])            # (7, 5, 9, 1, 20), (33, 17, 17, 1, 20), (6, 5, 17, 1, 3)
DETECTOR_PUBLISH = (DETECTOR[0], DETECTOR[1])                         # (7, 5, 9), (33, 17, 17)
RMSPROP_CASES = ((7, 5, 9, 1), (33, 17, 17, 1))                       # (H, C, T, scale), as the helper modules' GRAD_CASES
DECODER_REUSE, DETECTOR_REUSE = DECODER[10], DETECTOR[6]              # T = 513, T = 641: a long run, then 3 frames on the same handle
REUSE_FRAMES = 3
# (H, C, n, window) of the detector's trial in one call against its windows one by one: an exact multiple of the window, a trial
# below the window, windows of one frame, windows beyond both 256 and a remainder-free second one, and an odd size whose last
# window is a remainder of 3
DETECTOR_TRIALS = ((16, 8, 100, 50), (16, 8, 49, 50), (16, 8, 3, 1), (16, 8, 600, 300), (7, 5, 19, 8))
# the group forms at (7, 5): the members' trial lengths
DECODER_GROUP_FRAMES, DECODER_GROUP_MAX_FRAMES = (8, 9, 257), 257
DETECTOR_GROUP_FRAMES, DETECTOR_GROUP_WINDOW = (16, 17, 300), 8


def case(e: Entry):
    """(H, C, T, scale): what the helper modules' ``case_inputs`` take."""
    return (e.H, e.C, e.T, e.scale)


def ident(e: Entry) -> str:
    return "-".join(str(v) for v in e[:5] if v is not None)


def _mask(kind, random_mask, shape):
    if kind == "twos":
        return np.full(shape, 2.0, np.float32)
    assert kind in (None, "random"), kind
    return random_mask if kind else None


@functools.lru_cache(maxsize=None)
def decoder_inputs(e: Entry, mask):
    """state_dict (O outputs), x (T, C), y (T, O), mask (T, 2H) or None of a decoder entry.  Shared by the tests: not to be written to."""
    sd, x, y, m = D.case_inputs(case(e), "random", outputs=e.O)
    m = _mask(mask, m, (e.T, 2 * e.H))
    return sd, x, y, m


@functools.lru_cache(maxsize=None)
def detector_inputs(e: Entry, mask):
    """state_dict, x (T, C), y (T,), (h, c) [2][H], mask (T, H) or None of a detector entry.  Shared by the tests: not to be written to."""
    sd, x, y, state, m = V.case_inputs(case(e), "random")
    m = _mask(mask, m, (e.T, e.H))
    return sd, x, y, state, m


@functools.lru_cache(maxsize=None)
def decoder_truth(e: Entry, mask):
    """``D.autograd_trial`` in float64 on the entry's inputs: (loss, gradients, features), computed once."""
    return D.autograd_trial(*decoder_inputs(e, mask))


@functools.lru_cache(maxsize=None)
def detector_truth(e: Entry, mask):
    """``V.autograd_window`` in float64 on the entry's inputs: (loss, gradients, (h, c)), computed once."""
    return V.autograd_window(*detector_inputs(e, mask))


def float32_error(e: Entry, mask):
    """torch float32 CPU autograd against float64 on the entry's inputs: ({tensor: max|g32 - g64| / max|g64|}, the worst one's
    name).  The table's condition is that every figure stays within ``GRAD_BOUND / 4``."""
    import torch
    if e.O is None:
        err = V.rel_errors(V.autograd_window(*detector_inputs(e, mask), dtype=torch.float32)[1], detector_truth(e, mask)[1])
    else:
        err = D.rel_errors(D.autograd_trial(*decoder_inputs(e, mask), dtype=torch.float32)[1], decoder_truth(e, mask)[1])
    return err, max(err, key=err.get)


def runs(table):
    """[(entry, mask)] of a table, for parametrised tests."""
    return [(e, mask) for e in table for mask in e.masks]


def run_id(run) -> str:
    return f"{ident(run[0])}-{run[1] or 'nomask'}"
