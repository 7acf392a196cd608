#!/usr/bin/env python3
"""Time the lagged audio-ECoG spectrogram correlations of the acoustic contamination analysis at the size of one recording day:
64 channels x 3 000 000 samples at 1 kHz, the driver script's operator (200 ms frames at 50 Hz, 70-170 Hz, all 51 lags), seeded
noise.  (i) one `ContaminationGPU.moments_torch` call on device-resident signals, warm: median and interquartile range over
--reps repetitions after --warmup, each closed by a device synchronisation; (ii) the numpy statement of the method
(tests/contamination_reference.py) on the first tenth of the data on this machine's CPU, once, scaled by ten and labelled as
scaled.  Writes profiles/contamination.json and the measured paragraph of DESIGN.md section 5 (everything between the two
contamination-time markers is replaced; the device is named as the runtime names it).  `--prof` runs only five calls, for a
`rocprofv3 --kernel-trace --stats` run of its own; `--design-only` measures nothing and writes the paragraph from the JSON file.

    python tools/contamination_time.py [--reps 20] [--warmup 3] [--prof] [--no-numpy] [--no-design] [--design-only]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "delayed-speech-synthesis_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

SEED, FS, CHANNELS, ROWS = 9400, 1000, 64, 3_000_000
BEGIN, END = "<!-- contamination-time:begin -->", "<!-- contamination-time:end -->"


def stats(ms):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": float(med), "iqr_ms": float(q3 - q1), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def numpy_reference(brain, audio):
    import contamination_reference as ref
    t0 = time.perf_counter()
    ref.Day(brain, audio, FS).correlations()
    return (time.perf_counter() - t0) * 1e3


def write_design(res):
    path = os.path.join(ROOT, "DESIGN.md")
    text = open(path).read()
    d = res["one_call_device_resident"]
    para = (f"Measured by `tools/contamination_time.py` on {res['device']}: one `ContaminationGPU.moments_torch` call on "
            f"device-resident signals, {res['channels']} channels x {res['rows']} samples at 1 kHz ({res['frames']} frames), all "
            f"{res['lags']} lags, warm: **median {d['median_ms']:.1f} ms** (interquartile range {d['iqr_ms']:.2f} ms, "
            f"{d['n']} repetitions after {res['warmup']} warm-ups, each closed by a device synchronisation).")
    if "numpy_reference_cpu" in res:
        c = res["numpy_reference_cpu"]
        para += (f"  The numpy statement of the method took {c['ms_tenth']:.0f} ms for the first tenth of the data on that machine's "
                 f"CPU ({c['threads']} threads, one run): **{c['ms_scaled']:.0f} ms scaled** linearly to the whole day -- a scaled "
                 "figure, not a measurement of the whole.")
    new = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), BEGIN + "\n" + para + "\n" + END, text, flags=re.S)
    if new == text and para not in text:
        raise SystemExit("DESIGN.md has no contamination-time markers")
    open(path, "w").write(new)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--no-design", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contamination.json"))
    ap.add_argument("--design-only", action="store_true")
    a = ap.parse_args()
    if a.design_only:
        write_design(json.load(open(a.out)))
        return
    import torch
    from dss_amd.contamination import ContaminationGPU

    rng = np.random.default_rng(SEED)
    brain = rng.standard_normal((ROWS, CHANNELS))
    audio = 4.0 * rng.standard_normal(ROWS)
    d_brain, d_audio = torch.from_numpy(brain).cuda(), torch.from_numpy(audio).cuda()
    op = ContaminationGPU(FS)

    def call():
        m = op.moments_torch(d_brain, d_audio)
        torch.cuda.synchronize()
        return m

    if a.prof:
        for _ in range(5):
            call()
        return
    for _ in range(a.warmup):
        call()
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    res = {"seed": SEED, "channels": CHANNELS, "rows": ROWS, "frames": op.frames(ROWS), "lags": 2 * op.max_lag + 1, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "one_call_device_resident": stats(ms)}
    op.close()
    if not a.no_numpy:
        t = numpy_reference(brain[:ROWS // 10], audio[:ROWS // 10])
        res["numpy_reference_cpu"] = {"ms_tenth": t, "ms_scaled": 10 * t, "scaled": True, "n": 1,
                                      "threads": int(os.environ.get("OMP_NUM_THREADS", "0"))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if not a.no_design:
        write_design(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
