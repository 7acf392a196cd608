#!/usr/bin/env python3
"""Time the stream form of the LPC feature encoder (Part 18), audio resident on the device before the clock starts, features
left on the device.  Three shapes:

  ``packets``   128 streams x 4 frames per push (a microphone beside 40 ms ECoG packets), --pushes pushes back to back;
  ``xiph``      1 stream x 1 frame per push, the xiph call: the same device form, and the wall time of
                lpcnet_compute_single_frame_features through ctypes (host buffers, one frame in, 36 floats out);
  ``trials``    300 streams x 100 frames in ONE push, next to ``features_trials`` (Part 16, three launches) on the same audio and
                checked to give the same bits.

Per shape, --warmup repetitions, then --reps timed ones; median and min-max of
  ``device_ms``  between two events around the pushes, per push,
  ``wall_ms``    the host's clock from the first call until the device is idle, per push.

Writes profiles/feature_encoder_stream.json.  Nothing gates on these numbers.
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


def timed(torch, fn, calls, warmup, reps):
    """fn() issues `calls` calls; (device ms per call, wall ms per call) over reps repetitions."""
    dev, wall = [], []
    for rep in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3 / calls)
            dev.append(e0.elapsed_time(e1) / calls)
    return {"device_ms": stats(dev), "wall_ms": stats(wall), "calls_per_repetition": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pushes", type=int, default=100)
    ap.add_argument("--seed", type=int, default=9800)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_encoder_stream.json"))
    a = ap.parse_args()
    import torch
    from dss_amd import _lib
    from dss_amd.feature_encoder import LpcFeatureEncoderGPU, LpcFeatureStreamsGPU
    from dss_amd.synthetic import synthetic_speech_audio

    res = {"device": torch.cuda.get_device_name(0), "seed": a.seed}

    def shape(S, K):
        host = synthetic_speech_audio(a.seed + S, S * K * 160).reshape(S, K * 160)
        return host, torch.from_numpy(host).cuda(), LpcFeatureStreamsGPU(S)

    # 128 streams x 4 frames, and 1 stream x 1 frame: pushes back to back on the current stream
    for key, S, K in (("packets", 128, 4), ("xiph", 1, 1)):
        host, dev, st = shape(S, K)
        r = timed(torch, lambda: [st.push_torch(dev, total=True) for _ in range(a.pushes)], a.pushes, a.warmup, a.reps)
        r.update(streams=S, frames_per_push=K)
        res[key] = r
        st.close()

    # the xiph call itself through ctypes: host buffers, complete on return
    L = _lib.load()
    os.environ["DSS_LPCNET_ENCODER"] = "1"
    enc = L.lpcnet_encoder_create()
    if not enc:
        raise SystemExit(L.dss_last_error().decode())
    pcm = synthetic_speech_audio(a.seed, 160)
    f36 = np.zeros(36, np.float32)
    wall = []
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        for _ in range(a.pushes):
            assert L.lpcnet_compute_single_frame_features(enc, pcm.ctypes.data, f36.ctypes.data) == 0
        if rep >= a.warmup:
            wall.append((time.perf_counter() - t0) * 1e3 / a.pushes)
    L.lpcnet_encoder_destroy(enc)
    res["xiph"]["ctypes_call_wall_ms"] = stats(wall)

    # 300 streams x 100 frames in one push, beside the trial-list form on the same audio
    S, K = 300, 100
    host, dev, st = shape(S, K)
    flat = dev.reshape(-1)
    offsets = np.arange(S + 1, dtype=np.int64) * (K * 160)
    tl = LpcFeatureEncoderGPU()

    def one_push():
        st.reset()
        return st.push_torch(dev, total=True)

    same = bool(torch.equal(one_push().reshape(-1, 36), tl.features_trials_torch(flat, offsets, total=True)[0]))
    r = timed(torch, one_push, 1, a.warmup, a.reps)
    r.update(streams=S, frames_per_push=K, equal_bits_to_features_trials=same,
             features_trials=timed(torch, lambda: tl.features_trials_torch(flat, offsets, total=True), 1, a.warmup, a.reps))
    r["stream_over_trial_list_device"] = r["device_ms"]["median_ms"] / r["features_trials"]["device_ms"]["median_ms"]
    res["trials"] = r
    st.close()
    tl.close()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
