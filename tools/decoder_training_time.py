#!/usr/bin/env python3
"""Time the decoder's training on the GPU: ``DecoderTrainerGPU.train_trial`` (csrc/dec_train.hip) against the script's own loop
(train_bidirectional_model.py:134-152) on ``torch.nn.LSTM`` on the same GPU -- what a user had before the kernels.

  * one trial of 1500 frames, H = 100, C = 64, O = 20, dropout 0.5;
  * one epoch over --trials trials of 250 ... 1500 frames (2.5 - 15 s at 10 ms per frame), drawn with --seed.

Frames and targets are device-resident before the clock starts for both sides; wall clock with the device idle before and after;
--reps repetitions after --warmup, median and min-max.  Writes profiles/decoder_training.json.

    python tools/decoder_training_time.py [--trials 300] [--reps 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/decoder_training_time.py --prof
    python tools/decoder_training_time.py --summarize DIR        # adds the kernels' rows of DIR's kernel stats / trace to the JSON

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
    """The rows of dec_train_* kernels in a rocprofv3 --kernel-trace --stats CSV output directory."""
    res = json.load(open(out)) if os.path.exists(out) else {}
    prof = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "dec_train" in row.get("Name", ""):
                prof.setdefault(row["Name"].split("(")[0], {}).update(
                    calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Kernel_Name", "")
            if "dec_train" in name:
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=9500)
    ap.add_argument("--trials", type=int, default=300)
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_training.json"))
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.out)
    import torch
    import lstm_reference as R
    from dss_amd.models import BidirectionalSpeechSynthesisModel
    from dss_amd.training import DecoderTrainerGPU, decoder_dropout_mask

    C, H, O = 64, 100, 20
    sd = R.decoder_state_dict(H, C, 1)
    rng = np.random.default_rng(a.seed)
    lengths = [1500] + rng.integers(250, 1501, a.trials).tolist()
    xs = [torch.from_numpy(R.frames("x2", 1, n, C, a.seed + k)[0].astype(np.float32)).cuda() for k, n in enumerate(lengths)]
    ys = [torch.from_numpy(rng.standard_normal((n, O)).astype(np.float32)).cuda() for n in lengths]
    gen = torch.Generator().manual_seed(a.seed)
    masks = [decoder_dropout_mask(n, H, 0.5, gen).cuda() for n in lengths]
    tr = DecoderTrainerGPU(sd, max_frames=1500)

    def kernel_trials(idx):
        for k in idx:
            tr.train_trial(xs[k], ys[k], mask=masks[k])

    if a.prof:
        kernel_trials([0, 0, 0])
        torch.cuda.synchronize()
        return

    model = BidirectionalSpeechSynthesisModel(nb_layer=2, nb_hidden_units=H, nb_electrodes=C, dropout=0.5)
    model.load_state_dict(sd)
    model = model.cuda().train()
    optim = torch.optim.RMSprop(model.parameters(), lr=0.0001)
    cfunc = torch.nn.MSELoss(reduction="mean")

    def torch_trials(idx):                                   # the script's lines 134-155
        for k in idx:
            init_state = model.create_new_initial_state(batch_size=1, device="cuda")
            for param in model.parameters():
                param.grad = None
            pred, _ = model(xs[k][None], state=init_state)
            loss = cfunc(pred, ys[k][None])
            loss.backward()
            optim.step()
            loss.item()

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
    res = {"seed": a.seed, "H": H, "C": C, "O": O, "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "epoch_trials": a.trials, "epoch_frames": int(sum(lengths[1:])),
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
