#!/usr/bin/env python3
"""Time the LPC feature encoder (Part 16) on a session's worth of audio: --trials trials of mixed 1 ... 4 s at 16 kHz, int16 audio
resident on the device before the clock starts, features left on the device.

--warmup repetitions, then --reps timed ones; median and min-max of
  ``wall_ms``    the host's clock from the call until the device is idle,
  ``events_ms``  between two events around the call,
  ``launch_ms``  the device time of each of the three launches (the library's own events between them): spectrum / cepstrum /
                 LPC, residual and scores, pitch track -- and the track's share of their sum.  The track is serial per trial.

Merges its result into profiles/feature_encoder.json.  Nothing gates on these numbers.
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
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=9700)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_encoder.json"))
    a = ap.parse_args()
    import torch
    from dss_amd.feature_encoder import LpcFeatureEncoderGPU
    from dss_amd.synthetic import synthetic_speech_audio

    rng = np.random.default_rng(a.seed)
    lengths = rng.integers(16000, 64001, a.trials)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    audio = torch.from_numpy(synthetic_speech_audio(a.seed, int(offsets[-1]))).cuda()
    enc = LpcFeatureEncoderGPU()
    enc.enable_timing(True)
    wall, ev, launch = [], [], [[], [], []]
    frames = 0
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out, fo = enc.features_trials_torch(audio, offsets, total=True)
        e1.record()
        torch.cuda.synchronize()
        if rep < a.warmup:
            continue
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(e0.elapsed_time(e1))
        for k, ms in enumerate(enc.kernel_ms()):
            launch[k].append(ms)
        frames = int(fo[-1])
    med = [float(np.median(v)) for v in launch]
    res = {"device": torch.cuda.get_device_name(0), "trials": a.trials, "samples": int(offsets[-1]), "frames": frames, "seed": a.seed,
           "wall_ms": stats(wall), "events_ms": stats(ev),
           "launch_ms": {"spectrum_cepstrum_lpc": stats(launch[0]), "residual_scores": stats(launch[1]), "pitch_track": stats(launch[2])},
           "pitch_track_share_of_launches": med[2] / sum(med), "frames_per_second": frames / (float(np.median(ev)) / 1e3)}
    enc.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
