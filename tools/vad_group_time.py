#!/usr/bin/env python3
"""Time several detectors trained at once: ``VadGroupTrainerGPU.train_trials`` (the group kernels of csrc/vad_train.hip) against
the same number of single-trainer trials issued one after the other -- the single trainer's code path, timed in the same process.

H = 150, C = 64, dropout 0.5, windows of 50 frames, float32 frames, labels and (for the device clock) masks resident on the device
before the clock starts.

  (a) one trial step of M x 1500 frames (30 windows), M = 1, 8, 64, against M single trials of 1500 frames enqueued back to back on
      the same stream.  The single side is ``dss_vad_trainer_trial_dev`` -- what ``VadTrainerGPU.train_trial`` enqueues -- without
      train_trial's read-back of the losses, so that neither side waits for the host between trials.  Device time between two
      events on the stream.
  (b) one epoch of --trials trials of 100 ... 1500 frames per model at M = 8 through the stepping path of ``train_vads``
      (``_group_epoch`` over every model's own shuffled order, ``train_trials`` per step), against one single-trainer epoch over
      the same trials through ``train_vad``'s stepping path (``train_trial`` per trial); 8 sequential runs cost 8 times that.
      With host masks (each model's ``torch.Generator``) and with ``mask_source="device"``.  Wall clock around a final synchronise.

--reps repetitions (at least 7) after --warmup, median and min-max.  Writes profiles/vad_group.json.

    python tools/vad_group_time.py [--part a|b|all] [--trials 300] [--reps 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/vad_group_time.py --prof
    python tools/vad_group_time.py --summarize DIR       # adds the kernels' rows of DIR's kernel stats / trace to the JSON

--prof runs only (a)'s calls, once per M and three single trials, for a kernel trace in a run of its own.
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

WIDTHS = (1, 8, 64)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def summarize(d, out):
    """The rows of the vad_train_* and vad_group_* kernels in a rocprofv3 --kernel-trace --stats CSV output directory; the group
    kernels' launches also per grid (the trace has one row per launch), since one run holds M = 1, 8 and 64."""
    res = json.load(open(out)) if os.path.exists(out) else {}
    prof, per_grid = {}, {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "vad_train" in row.get("Name", "") or "vad_group" in row.get("Name", ""):
                prof.setdefault(row["Name"].split("(")[0], {}).update(
                    calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Kernel_Name", "")
            if "vad_train" in name or "vad_group" in name:
                k = prof.setdefault(name.split("(")[0], {})
                for src, dst in (("VGPR_Count", "vgpr"), ("Accum_VGPR_Count", "agpr"), ("SGPR_Count", "sgpr"), ("LDS_Block_Size", "lds_bytes"),
                                 ("Scratch_Size", "scratch_bytes")):
                    if src in row:
                        k[dst] = int(row[src])
                if "Start_Timestamp" in row and "End_Timestamp" in row and "Grid_Size_Y" in row and "Workgroup_Size_Y" in row:
                    models = int(row["Grid_Size_Y"]) // max(1, int(row["Workgroup_Size_Y"]))
                    per_grid.setdefault(f"{name.split('(')[0]} M={models}", []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    res["rocprofv3_kernel_trace"] = prof
    res["rocprofv3_per_width_us"] = {k: {"calls": len(v), "average_us": float(np.mean(v)), "median_us": float(np.median(v)),
                                         "min_us": float(np.min(v)), "max_us": float(np.max(v))} for k, v in sorted(per_grid.items())}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"kernels": prof, "per_width": res["rocprofv3_per_width_us"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("a", "b", "all"), default="all")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=9600)
    ap.add_argument("--trials", type=int, default=300)
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_group.json"))
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.out)
    if a.reps < 7:
        ap.error("--reps must be at least 7")
    import torch
    import lstm_reference as R
    from dss_amd import _lib
    from dss_amd.training import ALPHA, EPS, LR, DeviceMaskSource, VadGroupTrainerGPU, VadTrainerGPU, _group_epoch, dropout_mask

    C, H, W = 64, 150, 50
    sd = R.vad_state_dict(H, C, 1)
    rng = np.random.default_rng(a.seed)
    lengths = [1500] + rng.integers(100, 1501, a.trials).tolist()
    n_res = 1 if a.part == "a" or a.prof else len(lengths)
    xs = [torch.from_numpy(R.frames("x2", 1, n, C, a.seed + k)[0].astype(np.float32)).cuda() for k, n in enumerate(lengths[:n_res])]
    ys_host = [np.repeat(rng.integers(0, 2, n // 25 + 1), 25)[:n].astype(np.uint8) for n in lengths[:n_res]]
    ys = [torch.from_numpy(y).cuda() for y in ys_host]    # the group takes resident labels (train_vads); train_vad uploads per trial
    gen = torch.Generator().manual_seed(a.seed)
    dmask = dropout_mask(1500, H, 0.5, gen).cuda()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    single = VadTrainerGPU(sd, max_window=W)
    single_losses = torch.empty((30,), dtype=torch.float64, device="cuda")
    groups = {}

    def group(M):
        if M not in groups:
            groups.clear()                                                             # one group's workspace at a time
            groups[M] = VadGroupTrainerGPU([sd] * M, max_window=W)
        return groups[M]

    def timed(fn, clock):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) if clock == "device" else (time.perf_counter() - t0) * 1e3)
        return stats(ms)

    # (a) one trial step of M x 1500 frames
    def single_trials(M):
        def fn():
            for _ in range(M):                             # train_trial's launches, without its read-back
                _lib.check(single._L.dss_vad_trainer_trial_dev(single._h, xs[0].data_ptr(), 0, 1500, ys[0].data_ptr(), dmask.data_ptr(), W, LR, ALPHA,
                                                               EPS, single_losses.data_ptr(), stream()))
        return fn

    def group_step(M):
        g = group(M)
        losses = torch.empty((M, 30), dtype=torch.float64, device="cuda")
        return lambda: g.train_trials([xs[0]] * M, [ys[0]] * M, W, [dmask] * M, losses=losses)

    if a.prof:
        for M in WIDTHS:
            group_step(M)()
        for _ in range(3):
            single_trials(1)()
        torch.cuda.synchronize()
        return

    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.update({"seed": a.seed, "H": H, "C": C, "window": W, "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup})
    if a.part in ("a", "all"):
        step = {}
        for M in WIDTHS:
            s, g = timed(single_trials(M), "device"), timed(group_step(M), "device")
            spread = s["max_ms"] - s["min_ms"]
            r = {"single_trials_in_sequence_device": s, "group_step_device": g, "sequence_over_group": s["median_ms"] / g["median_ms"],
                 "single_spread_ms": spread, "group_ms_per_model": g["median_ms"] / M}
            step[str(M)] = r
            print(M, json.dumps(r), flush=True)
        one = step["1"]["single_trials_in_sequence_device"]
        spread1 = one["max_ms"] - one["min_ms"]
        step["acceptance"] = {
            "M8_group_below_8_singles_by_more_than_their_spread":
                step["8"]["single_trials_in_sequence_device"]["median_ms"] - step["8"]["group_step_device"]["median_ms"] > step["8"]["single_spread_ms"],
            "M1_group_within_the_spread_of_one_single_trial": abs(step["1"]["group_step_device"]["median_ms"] - one["median_ms"]) <= spread1,
            "M1_group_minus_single_ms": step["1"]["group_step_device"]["median_ms"] - one["median_ms"], "one_single_trial_spread_ms": spread1}
        print("acceptance", json.dumps(step["acceptance"]), flush=True)
        res["trial_step_1500_frames"] = step

    if a.part in ("b", "all"):
        n, M = a.trials, 8
        ep_len = [lengths[1:]]

        def single_epoch(device_masks):
            def fn():
                g1 = torch.Generator().manual_seed(a.seed + 1)
                src = DeviceMaskSource(a.seed + 1) if device_masks else None
                for k in torch.randperm(n, generator=g1).tolist():
                    single.train_trial(xs[1 + k], ys_host[1 + k], window=W, dropout=0.5, generator=src or g1)
            return fn

        def group_epoch(device_masks):
            g = group(M)

            def fn():
                gens = [torch.Generator().manual_seed(a.seed + 1 + m) for m in range(M)]
                sources = [DeviceMaskSource(a.seed + 1 + m) for m in range(M)] if device_masks else None

                def step(trials, masks):
                    return g.train_trials([None if k is None else xs[1 + k] for k in trials], [None if k is None else ys[1 + k] for k in trials], W, masks)

                _group_epoch(step, gens, [n] * M, ep_len * M, H, 0.5, True, sources, dropout_mask, H)
            return fn

        epoch = {"trials": n, "frames": int(sum(lengths[1:])), "windows": int(sum(-(-k // W) for k in lengths[1:])), "M": M}
        for name, dev in (("host_masks", False), ("device_masks", True)):
            s, g = timed(single_epoch(dev), "wall"), timed(group_epoch(dev), "wall")
            epoch[name] = {"single_trainer_epoch_wall": s, "group_epoch_wall": g, "M_sequential_epochs_over_group": M * s["median_ms"] / g["median_ms"]}
            print("epoch", name, json.dumps(epoch[name]), flush=True)
        res["epoch"] = epoch
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
