#!/usr/bin/env python3
"""Time the loudness step of the trial audio on the session of tools/acoustic_vad_time.py (300 trials of 1-4 s in a 10-minute
seeded wav, lead 256, every 17th trial a SILENCE trial), device-resident, with that tool's timer (wall clock around a
synchronised call): (i) the plain labels, (ii) the labels of the normalised audio (peak, energy, vote), (iii) the prepared
audio alone (peak, prepare), (iv) the same from host buffers.  Median and interquartile range over --reps repetitions after
--warmup; writes profiles/trial_audio.json.  `--prof` runs only five calls of (ii) and (iii), for a
`rocprofv3 --kernel-trace --stats` run of its own.

    python tools/trial_audio_time.py [--reps 20] [--warmup 3] [--prof]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "delayed-speech-synthesis_amd"))


def stats(ms):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": float(med), "iqr_ms": float(q3 - q1), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trial_audio.json"))
    a = ap.parse_args()
    import torch
    from dss_amd.acoustic_vad import AcousticVadGPU
    from dss_amd.synthetic import synthetic_speech_audio

    fs, n_audio = 16000, 600 * 16000
    wav = synthetic_speech_audio(8200, n_audio)
    rng = np.random.default_rng(8201)
    ranges = []
    for _ in range(300):
        n = int(rng.uniform(1.0, 4.0) * fs) + 640
        ranges.append((int(rng.integers(0, n_audio - n)), n))
    silence = [k % 17 == 3 for k in range(300)]
    v = AcousticVadGPU()
    v.set_gain()
    d_wav = torch.from_numpy(wav).cuda()

    def synced(fn):
        def run():
            out = fn()
            torch.cuda.synchronize()
            return out
        return run

    plain = synced(lambda: v.labels_trials_torch(d_wav, ranges, lead=256, silence=silence))
    normalised = synced(lambda: v.labels_trials_torch(d_wav, ranges, lead=256, silence=silence, normalize=True))
    audio = synced(lambda: v.prepared_audio_trials_torch(d_wav, ranges, lead=256, silence=silence, normalize=True))

    if a.prof:
        for _ in range(5):
            normalised()
            audio()
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

    res = {"trials": len(ranges), "frames": int(sum(v.trial_frames(n) for _, n in ranges)), "samples": int(sum(n for _, n in ranges)),
           "normalised_trials": int(300 - sum(silence)), "device": torch.cuda.get_device_name(0)}
    res["plain_labels_device_resident"] = timed(plain, a.reps, a.warmup)
    res["normalised_labels_device_resident"] = timed(normalised, a.reps, a.warmup)
    res["prepared_audio_device_resident"] = timed(audio, a.reps, a.warmup)
    res["normalised_labels_host_buffers"] = timed(lambda: v.labels_trials(wav, ranges, lead=256, silence=silence, normalize=True),
                                                  a.reps, a.warmup)
    res["prepared_audio_host_buffers"] = timed(lambda: v.prepared_audio_trials(wav, ranges, lead=256, silence=silence, normalize=True),
                                               a.reps, a.warmup)
    v.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
