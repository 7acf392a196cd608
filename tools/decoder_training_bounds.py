#!/usr/bin/env python3
"""Measure the gradient bounds of the decoder's training tests without a GPU.

For every case of tests/decoder_training_reference.GRAD_CASES, with and without a dropout mask, torch float32 CPU autograd is compared
with the float64 reference (``autograd_trial``) per tensor: max|g32 - g64| / max|g64|.  The bound of the GPU tests is 4 x the worst
of these figures, rounded up to one significant digit; it is stored as ``GRAD_BOUND`` in the helper module, and this tool says
whether the stored constant still equals what it measures.  The worst case of at most 50 frames and the 350-frame trial are
reported apart: were the long trial to set the bound far above the short cases, it would get a constant of its own.

The case table of tests/training_cases.py (odd sizes, frame tiles, long trials, output counts) is walked the same way and reported
beside it.  It does not set the bound: it has to fit it, 4 x its worst figure being at most the stored ``GRAD_BOUND``
(tests/test_cpu_training_cases.py asserts that per entry).

    python tools/decoder_training_bounds.py
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "delayed-speech-synthesis_amd")]


def round_up_1(x: float) -> float:
    e = math.floor(math.log10(x))
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


def main() -> int:
    import torch
    import decoder_training_reference as D
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    worst = {False: (0.0, None), True: (0.0, None)}
    for case in D.GRAD_CASES:
        for mask in (None, "random"):
            sd, x, y, m = D.case_inputs(case, mask)
            _, g64, _ = D.autograd_trial(sd, x, y, m)
            _, g32, _ = D.autograd_trial(sd, x, y, m, dtype=torch.float32)
            err = D.rel_errors(g32, g64)
            k = max(err, key=err.get)
            print(f"(H, C, T, scale) = {case}  mask = {mask!s:8}  worst tensor {k:30} {err[k]:.3g}")
            long = case[2] > 50
            if err[k] > worst[long][0]:
                worst[long] = (err[k], (case, mask, k))
    for long in (False, True):
        print(f"torch float32 worst, {'the 350-frame trial' if long else 'cases of at most 50 frames'}: {worst[long][0]:.3g} at {worst[long][1]}")
    w = max(worst[False][0], worst[True][0])
    bound = round_up_1(4.0 * w)
    print(f"4 x {w:.3g} = {4 * w:.3g}  ->  bound {bound:g}")
    print(f"stored GRAD_BOUND = {D.GRAD_BOUND:g}" + ("" if math.isclose(bound, D.GRAD_BOUND, rel_tol=1e-9) else "   (differs: this CPU's torch rounds differently, or the cases changed)"))
    import training_cases as TC
    table = (0.0, None)
    for e, mask in TC.runs(TC.DECODER):
        err, k = TC.float32_error(e, mask)
        print(f"(H, C, T, scale, O) = {tuple(e[:5])}  mask = {mask!s:8}  worst tensor {k:30} {err[k]:.3g}")
        if err[k] > table[0]:
            table = (err[k], (tuple(e[:5]), mask, k))
    fits = 4.0 * table[0] <= D.GRAD_BOUND
    print(f"torch float32 worst, the case table: {table[0]:.3g} at {table[1]}  (GRAD_CASES: {w:.3g})")
    print(f"4 x {table[0]:.3g} = {4 * table[0]:.3g}  " + (f"<= stored GRAD_BOUND = {D.GRAD_BOUND:g}: the table fits the bound" if fits else
                                                        f">  stored GRAD_BOUND = {D.GRAD_BOUND:g}: the table does NOT fit the bound; replace the entry"))
    return 0 if fits else 1


if __name__ == "__main__":
    sys.exit(main())
