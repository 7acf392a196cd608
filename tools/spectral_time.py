#!/usr/bin/env python3
"""Time the speech-locked spectral power of the reference's per-electrode analysis (eval/suppl_fig_2.py:41-92) at its own size:
128 channels at 1 kHz, 60 keyword trials of 2.5-4 s (plus the script's 1.5 s behind each) and 60 calibration trials in seeded
10-minute recordings:
(i) one speech_locked_power call on device-resident recordings, (ii) the same from host buffers, (iii) the scipy loop of the
script (one scipy.signal.spectrogram call per trial and channel) on this machine's CPU, one repetition.  Median and
interquartile range over --reps repetitions after --warmup for (i) and (ii); writes profiles/spectral.json.  `--prof` runs only
five device-resident calls, for a `rocprofv3 --kernel-trace --stats` run of its own.

    python tools/spectral_time.py [--reps 20] [--warmup 3] [--prof] [--no-scipy]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "delayed-speech-synthesis_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

SEED, FS, CHANNELS, ROWS, TRIALS = 9300, 1000, 128, 600 * 1000, 60


def stats(ms):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": float(med), "iqr_ms": float(q3 - q1), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def workload():
    rng = np.random.default_rng(SEED)
    cal = rng.standard_normal((ROWS, CHANNELS + 1))                                 # 129 columns, as the amplifier delivers them
    rec = rng.standard_normal((ROWS, CHANNELS + 1))
    cal_ranges, ranges, onsets = [], [], []
    for _ in range(TRIALS):
        n = int(rng.uniform(2.5, 4.0) * FS)
        cal_ranges.append((int(rng.integers(0, ROWS - n)), n))
        n = int(rng.uniform(2.5, 4.0) * FS) + int(1.5 * FS)
        ranges.append((int(rng.integers(0, ROWS - n)), n))
        onsets.append(int(rng.integers(50, (n - 50) // 10 + 1 - 150 + 1)))
    return cal, cal_ranges, rec, ranges, onsets


def scipy_loop(cal, cal_ranges, rec, ranges, onsets):
    from scipy.signal import spectrogram
    base = np.zeros((CHANNELS, 51), dtype=np.float32)
    out = np.zeros((CHANNELS, 51, 200), dtype=np.float32)
    for c in range(CHANNELS):
        b = [spectrogram(cal[a:a + n, c], fs=FS, window="hann", nfft=100, nperseg=50, noverlap=40)[2] for a, n in cal_ranges]
        base[c] = np.mean(np.concatenate(b, axis=1), axis=-1)
    for c in range(CHANNELS):
        cut = []
        for (a, n), o in zip(ranges, onsets):
            sxx = spectrogram(rec[a:a + n, c], fs=FS, window="hann", nfft=100, nperseg=50, noverlap=40)[2]
            cut.append(sxx[:, o - 50:o + 150])
        m = np.mean(np.stack(cut), axis=0)
        out[c] = 10 * np.log10(m / np.tile(base[c], (m.shape[1], 1)).T)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral.json"))
    a = ap.parse_args()
    import torch
    from dss_amd.spectral import speech_locked_power

    cal, cal_ranges, rec, ranges, onsets = workload()
    d_cal, d_rec = torch.from_numpy(cal).cuda(), torch.from_numpy(rec).cuda()

    def dev():
        return speech_locked_power(d_cal[:, :CHANNELS], cal_ranges, d_rec[:, :CHANNELS], ranges, onsets)   # ends in a copy to the host

    def host():
        return speech_locked_power(cal[:, :CHANNELS], cal_ranges, rec[:, :CHANNELS], ranges, onsets)

    if a.prof:
        for _ in range(5):
            dev()
        return

    def timed(fn, reps, warmup):
        for _ in range(warmup):
            fn()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms)

    frames = sum((n - 50) // 10 + 1 for _, n in ranges)
    cal_frames = sum((n - 50) // 10 + 1 for _, n in cal_ranges)
    res = {"seed": SEED, "channels": CHANNELS, "trials": TRIALS, "frames": int(frames), "calibration_frames": int(cal_frames),
           "device": torch.cuda.get_device_name(0)}
    res["one_call_device_resident"] = timed(dev, a.reps, a.warmup)
    res["one_call_host_buffers"] = timed(host, a.reps, a.warmup)
    got = dev()
    if not a.no_scipy:
        t0 = time.perf_counter()
        want = scipy_loop(cal, cal_ranges, rec, ranges, onsets)
        res["scipy_loop_cpu"] = {"ms": (time.perf_counter() - t0) * 1e3, "n": 1, "threads": int(os.environ.get("OMP_NUM_THREADS", "0"))}
        res["max_abs_difference_db"] = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
