#!/usr/bin/env python3
"""Time the acoustic VAD labels of a 300-trial session (trials of 1-4 s in a 10-minute seeded wav, lead 256):
(i) one call from host buffers, (ii) one call device-resident, (iii) one call per trial, (iv) the vectorised numpy
restatement (tests/acoustic_vad_reference.py) on this machine's CPU.  Median and interquartile range over --reps
repetitions after --warmup; writes profiles/acoustic_vad.json.  `--prof` runs only five device-resident calls, for a
`rocprofv3 --kernel-trace --stats` run of its own.

    python tools/acoustic_vad_time.py [--reps 20] [--warmup 3] [--prof]
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


def stats(ms):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": float(med), "iqr_ms": float(q3 - q1), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acoustic_vad.json"))
    a = ap.parse_args()
    import torch
    import acoustic_vad_reference as ref
    from dss_amd.acoustic_vad import AcousticVadGPU
    from dss_amd.synthetic import synthetic_speech_audio

    fs, n_audio = 16000, 600 * 16000
    wav = synthetic_speech_audio(8200, n_audio)
    rng = np.random.default_rng(8201)
    ranges = []
    for _ in range(300):
        n = int(rng.uniform(1.0, 4.0) * fs) + 640
        ranges.append((int(rng.integers(0, n_audio - n)), n))
    v = AcousticVadGPU()
    d_wav = torch.from_numpy(wav).cuda()
    frames = sum(v.trial_frames(n) for _, n in ranges)
    seconds = sum(n for _, n in ranges) / fs

    def dev():
        out = v.labels_trials_torch(d_wav, ranges, lead=256)
        torch.cuda.synchronize()
        return out

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

    res = {"trials": len(ranges), "frames": int(frames), "audio_seconds": seconds, "device": torch.cuda.get_device_name(0)}
    res["one_call_host_buffers"] = timed(lambda: v.labels_trials(wav, ranges, lead=256), a.reps, a.warmup)
    res["one_call_device_resident"] = timed(dev, a.reps, a.warmup)
    res["one_call_per_trial_host_buffers"] = timed(lambda: [v.labels_trials(wav, [r], lead=256) for r in ranges], max(a.reps // 4, 3), 1)

    def cpu():
        for first, n in ranges:
            ref.vote(ref.log_energy(ref.trial_samples(wav, first, n, 256), v.window_fn, v.mel))
    res["numpy_restatement_cpu"] = timed(cpu, 3, 0)
    res["numpy_restatement_cpu"]["threads"] = int(os.environ.get("OMP_NUM_THREADS", "0"))
    res["reference_class_ms_per_audio_second_on_the_development_machine"] = 7.0
    v.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
