#!/usr/bin/env python3
"""Time the detector's training on the GPU: ``VadTrainerGPU.train_trial`` (csrc/vad_train.hip) against the script's own loop
(train_unidirectional_vad.py:144-175) on ``torch.nn.LSTM`` on the same GPU -- what a user had before the kernels.

  * one trial of 1500 frames (30 windows of 50), H = 150, C = 64, dropout 0.5;
  * one epoch over --trials trials of 100 ... 1500 frames (1 - 15 s at 10 ms per frame), drawn with --seed.

Frames and targets are device-resident before the clock starts for both sides; wall clock with the device idle before and after;
--reps repetitions after --warmup, median and min-max.  Writes profiles/vad_training.json.

    python tools/vad_training_time.py [--trials 300] [--reps 3]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/vad_training_time.py --prof
    python tools/vad_training_time.py --summarize DIR        # adds the two kernels' rows of DIR's kernel stats / trace to the JSON

--prof runs only three 1500-frame trials through the kernels, for a kernel trace in a run of its own.
"""
import argparse
import csv
import glob
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


def summarize(d, out):
    """The rows of vad_train_* kernels in a rocprofv3 --kernel-trace --stats CSV output directory."""
    res = json.load(open(out)) if os.path.exists(out) else {}
    prof = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "vad_train" in row.get("Name", ""):
                prof.setdefault(row["Name"].split("(")[0], {}).update(
                    calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Kernel_Name", "")
            if "vad_train" in name:
                k = prof.setdefault(name.split("(")[0], {})
                for src, dst in (("VGPR_Count", "vgpr"), ("Accum_VGPR_Count", "agpr"), ("SGPR_Count", "sgpr"), ("LDS_Block_Size", "lds_bytes"),
                                 ("Scratch_Size", "scratch_bytes")):
                    if src in row:
                        k[dst] = int(row[src])
    res["rocprofv3_kernel_trace"] = prof
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(prof))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=9400)
    ap.add_argument("--trials", type=int, default=300)
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_training.json"))
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.out)
    import torch
    import lstm_reference as R
    from dss_amd.models import UnidirectionalVoiceActivityDetector
    from dss_amd.training import VadTrainerGPU, dropout_mask

    C, H, W = 64, 150, 50
    sd = R.vad_state_dict(H, C, 1)
    rng = np.random.default_rng(a.seed)
    lengths = [1500] + rng.integers(100, 1501, a.trials).tolist()
    xs = [torch.from_numpy(R.frames("x2", 1, n, C, a.seed + k)[0].astype(np.float32)).cuda() for k, n in enumerate(lengths)]
    ys = [np.repeat(rng.integers(0, 2, n // 25 + 1), 25)[:n].astype(np.uint8) for n in lengths]
    yd = [torch.from_numpy(y).cuda().long() for y in ys]
    gen = torch.Generator().manual_seed(a.seed)
    masks = [dropout_mask(n, H, 0.5, gen).cuda() for n in lengths]
    tr = VadTrainerGPU(sd, max_window=W)

    def kernel_trials(idx):
        for k in idx:
            tr.train_trial(xs[k], ys[k], window=W, masks=masks[k])

    if a.prof:
        kernel_trials([0, 0, 0])
        torch.cuda.synchronize()
        return

    model = UnidirectionalVoiceActivityDetector(nb_layer=2, nb_hidden_units=H, nb_electrodes=C, dropout=0.5)
    model.load_state_dict(sd)
    model = model.cuda().train()
    optim = torch.optim.RMSprop(model.parameters(), lr=0.0001)
    cfunc = torch.nn.CrossEntropyLoss()

    def torch_trials(idx):                                   # the script's lines 144-175
        for k in idx:
            state = model.create_new_initial_state(batch_size=1, device="cuda")
            losses = []
            for x_seq, y_seq in zip(xs[k][None].split(W, dim=1), yd[k][None].split(W, dim=1)):
                for param in model.parameters():
                    param.grad = None
                output, state = model(x_seq, state)
                loss = cfunc(torch.reshape(output, (-1, 2)), y_seq.reshape(-1))
                loss.backward()
                optim.step()
                state = (state[0].detach(), state[1].detach())
                losses.append(loss.item())

    def timed(fn, idx):
        for _ in range(a.warmup):
            fn(idx[:3])
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(idx)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms)

    epoch = list(range(1, len(lengths)))
    res = {"seed": a.seed, "H": H, "C": C, "window": W, "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "epoch_trials": a.trials, "epoch_frames": int(sum(lengths[1:])), "epoch_windows": int(sum(-(-n // W) for n in lengths[1:])),
           "trial_1500_frames": {"train_trial": timed(kernel_trials, [0]), "torch_loop": timed(torch_trials, [0])},
           "epoch": {"train_trial": timed(kernel_trials, epoch), "torch_loop": timed(torch_trials, epoch)}}
    for k in ("trial_1500_frames", "epoch"):
        res[k]["torch_over_kernels"] = res[k]["torch_loop"]["median_ms"] / res[k]["train_trial"]["median_ms"]
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        if "rocprofv3_kernel_trace" in old:
            res["rocprofv3_kernel_trace"] = old["rocprofv3_kernel_trace"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
