#!/usr/bin/env python3
"""Time the validation pass of M models trained side by side, both ways, in one run:

  (a) the per-model path as ``train_decoders`` / ``train_vads`` run it by default: for every model, publish the member into one
      kept inference handle, then ``decoder_validation`` / ``vad_validation`` on the model's corpus (host arrays: the frames are
      uploaded again, the trial-list forward, one score launch, the scores to the host);
  (b) one ``decoder_validation_group`` / ``vad_validation_group`` call on a ``GroupValidationSet`` prepared before the clock starts.

The corpus shape of tools/decoder_group_time.py: C = 64, H = 100 (decoder, 20 outputs) / 150 (detector), 30 validation trials of
250 ... 1500 frames per model, float32 frames; M = 1, 8 and 64.  Two clocks around each call: ``wall_ms`` (the host's clock until
the device is idle and the results are host arrays) and ``device_ms`` (between two events on the stream).  --reps repetitions
after --warmup, median and min-max.  Writes profiles/group_validation.json.

    python tools/group_validation_time.py [--reps 10] [--warmup 2] [--models 1 8 64]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=9700)
    ap.add_argument("--trials", type=int, default=30)
    ap.add_argument("--models", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_validation.json"))
    a = ap.parse_args()
    import torch
    import lstm_reference as R
    from dss_amd import validation
    from dss_amd.decoder import BiLstmDecoderGPU
    from dss_amd.training import DecoderGroupTrainerGPU, VadGroupTrainerGPU
    from dss_amd.vad import VadLstmGPU

    C, O = 64, 20
    rng = np.random.default_rng(a.seed)

    def corpus(kind):
        lengths = rng.integers(250, 1501, a.trials)
        n = int(lengths.sum())
        c = dict(hga_activity=rng.standard_normal((n, C), dtype=np.float32) * np.float32(2.0), trial_ids=np.repeat(np.arange(a.trials), lengths))
        if kind == "decoder":
            c["lpc_coefficients"] = rng.standard_normal((n, O), dtype=np.float32)
        else:
            c["vad_labels"] = np.repeat(rng.integers(0, 2, n // 20 + 1), 20)[:n].astype(np.uint8)
        return c, lengths

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        wall, dev = [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
        return {"wall_ms": stats(wall), "device_ms": stats(dev)}

    res = {"seed": a.seed, "C": C, "O": O, "trials_per_model": a.trials, "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "warmup": a.warmup, "decoder": {"H": 100}, "vad": {"H": 150}}
    for kind, H in (("decoder", 100), ("vad", 150)):
        sd = R.decoder_state_dict(H, C, 1) if kind == "decoder" else R.vad_state_dict(H, C, 1)
        for M in a.models:
            made = [corpus(kind) for _ in range(M)]
            corpora, longest = [c for c, _ in made], int(max(n.max() for _, n in made))
            frames = int(sum(n.sum() for _, n in made))
            if kind == "decoder":
                group = DecoderGroupTrainerGPU([sd] * M, max_frames=longest)
                handle = BiLstmDecoderGPU(a.trials, longest, state_dict=sd)        # as train_decoders sizes it: min(trials, 256) streams

                def per_model():
                    for m, c in enumerate(corpora):
                        group.publish(m, handle)
                        validation.decoder_validation(handle, c["hga_activity"], c["lpc_coefficients"], c["trial_ids"])
            else:
                group = VadGroupTrainerGPU([sd] * M, max_window=50)
                handle = VadLstmGPU(1, state_dict=sd)

                def per_model():
                    for m, c in enumerate(corpora):
                        group.publish(m, handle)
                        validation.vad_validation(handle, c["hga_activity"], c["vad_labels"], c["trial_ids"])
            vset = validation.GroupValidationSet(corpora, kind)
            one_call = validation.decoder_validation_group if kind == "decoder" else validation.vad_validation_group
            r = {"frames": frames, "longest_trial": longest, "per_model": timed(per_model), "group": timed(lambda: one_call(group, vset))}
            for clock in ("wall_ms", "device_ms"):
                r[f"per_model_over_group_{clock[:-3]}"] = r["per_model"][clock]["median_ms"] / r["group"][clock]["median_ms"]
            res[kind][str(M)] = r
            print(kind, M, json.dumps(r), flush=True)
            del group, handle, vset
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
