#!/usr/bin/env python3
"""Measure the log-energy bounds of the acoustic VAD case tests without a GPU.

For every geometry case of tests/acoustic_vad_cases.py the float64 restatement (tests/acoustic_vad_reference.py, fed the
package's own window and mel matrix) is compared with tests/golden/acoustic_vad_cases.npz, which the reference's EnergyBasedVad
computed: D = max |restatement - fixture| over the case's four trials, U = one ulp of the case's largest |log energy|, and the
bound of the GPU test is 4 x max(D, U).  The kernel's figure never enters.  The tool prints D, U and the bound per case and says
whether the constants stored in the case module still cover what it measures (a stored D is the largest figure seen on the CPUs
the tool ran on, so a smaller measurement is fine and a larger one is reported).

    python tools/acoustic_vad_bounds.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "delayed-speech-synthesis_amd")]


def measure(g):
    """{case: (D, U, frames)} from the loaded fixture."""
    import acoustic_vad_cases as vc
    import acoustic_vad_reference as ref
    from dss_amd import acoustic_vad
    out = {}
    pos = 0
    for c in vc.GEOMETRY:
        win, mel = acoustic_vad.hann(c.N), acoustic_vad.mel_filterbank(c.bins, c.n_bands, c.fs)
        wav = vc.audio(c.name)
        D, first_frame = 0.0, pos
        for first, n in vc.trials(c.name):
            le = ref.log_energy(ref.trial_samples(wav, first, n, 0), win, mel, shift=c.shift)
            D = max(D, float(np.max(np.abs(le - g["log_energy"][pos:pos + len(le)]))))
            pos += len(le)
        out[c.name] = (D, vc.ulp_of_largest(g["log_energy"][first_frame:pos]), pos - first_frame)
    assert pos == len(g["log_energy"])
    return out


def main() -> int:
    import acoustic_vad_cases as vc
    g = np.load(os.path.join(ROOT, "tests", "golden", "acoustic_vad_cases.npz"), allow_pickle=False)
    differs = False
    for name, (D, U, frames) in measure(g).items():
        c = vc.case(name)
        note = ""
        if D > c.D or U != vc.U.get(name):
            differs = True
            note = "   (stored D = %.3g, U = %.3g: not covered)" % (c.D, vc.U.get(name, float("nan")))
        b = vc.MARGIN * max(D, U)
        print(f"{name:18} frames {frames:4}  D = {D:.3e}  U = {U:.3e}  4 x max = {b:.3e}  stored bound "
              f"{vc.MARGIN * max(c.D, vc.U.get(name, 0.0)):.3e}" + note)
        assert b <= vc.CAP, name
    print("the stored constants cover this CPU's figures" if not differs
          else "differs: this CPU's numpy rounds differently, or the cases changed")
    return 0


if __name__ == "__main__":
    sys.exit(main())
