#!/usr/bin/env python3
"""Time several decoders trained at once: ``DecoderGroupTrainerGPU.step`` (the group kernels of csrc/dec_train.hip) against the
same number of ``DecoderTrainerGPU`` trials issued one after the other -- the single trainer's code path, timed in the same session.

H = 100, C = 64, O = 20, dropout 0.5, float32 frames and targets resident on the device before the clock starts.

  (a) one step of M x 1500 frames, M = 1, 2, 4, 8, 16, 32, 64, against M single trials of 1500 frames;
  (b) one epoch of --trials trials of 250 ... 1500 frames per model for M = 1 and 8, every model in its own shuffled order (so the
      lengths mix within a step), against one single-trainer epoch over the same trials; M sequential runs cost M times that.

Two clocks for each:
  * ``device_ms``: between two events around the calls, with the masks already on the device -- the launches alone;
  * ``wall_ms``: the host's clock from before the masks are drawn (the CPU generator, as ``train_decoder`` / ``train_decoders`` draw
    them) until the device is idle -- what a training loop pays.  wall - device is the drawing and the upload of the masks.
--reps repetitions after --warmup, median and min-max.  Writes profiles/decoder_group.json.

    python tools/decoder_group_time.py [--trials 300] [--reps 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/decoder_group_time.py --prof
    python tools/decoder_group_time.py --summarize DIR       # adds the kernels' rows of DIR's kernel stats / trace to the JSON

--prof runs only three steps of 8 x 1500 frames and three single trials, for a kernel trace in a run of its own.
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

WIDTHS = (1, 2, 4, 8, 16, 32, 64)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def summarize(d, out):
    """The rows of the dec_train_* and dec_group_* kernels in a rocprofv3 --kernel-trace --stats CSV output directory."""
    res = json.load(open(out)) if os.path.exists(out) else {}
    prof = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "dec_train" in row.get("Name", "") or "dec_group" in row.get("Name", ""):
                prof.setdefault(row["Name"].split("(")[0], {}).update(
                    calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Kernel_Name", "")
            if "dec_train" in name or "dec_group" in name:
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_group.json"))
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.out)
    import torch
    import lstm_reference as R
    from dss_amd.training import DecoderGroupTrainerGPU, DecoderTrainerGPU, _group_epoch, decoder_dropout_mask

    C, H, O = 64, 100, 20
    sd = R.decoder_state_dict(H, C, 1)
    rng = np.random.default_rng(a.seed)
    lengths = [1500] + rng.integers(250, 1501, a.trials).tolist()
    xs = [torch.from_numpy(R.frames("x2", 1, n, C, a.seed + k)[0].astype(np.float32)).cuda() for k, n in enumerate(lengths)]
    ys = [torch.from_numpy(rng.standard_normal((n, O)).astype(np.float32)).cuda() for n in lengths]
    gen = torch.Generator().manual_seed(a.seed)
    dmasks = [decoder_dropout_mask(n, H, 0.5, gen).cuda() for n in lengths]           # masks on the device, for the device clock
    single = DecoderTrainerGPU(sd, max_frames=1500)
    groups = {}

    def group(M):
        if M not in groups:
            groups.clear()                                                             # one group's workspace at a time
            groups[M] = DecoderGroupTrainerGPU([sd] * M, max_frames=1500)
        return groups[M]

    def timed(fn):
        """fn(host_masks) runs once; device clock with masks resident, wall clock with masks drawn on the host."""
        out = {}
        for clock in ("device_ms", "wall_ms"):
            for _ in range(a.warmup):
                fn(clock == "wall_ms")
            ms = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                fn(clock == "wall_ms")
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) if clock == "device_ms" else (time.perf_counter() - t0) * 1e3)
            out[clock] = stats(ms)
        out["host_share_of_wall"] = 1.0 - out["device_ms"]["median_ms"] / out["wall_ms"]["median_ms"]
        return out

    # (a) one step of M x 1500 frames
    def single_trials(M):
        def fn(host_masks):
            for _ in range(M):
                m = decoder_dropout_mask(1500, H, 0.5, gen) if host_masks else dmasks[0]
                single._trial(xs[0], ys[0], m, True, 1e-4, 0.99, 1e-8)
        return fn

    def group_step(M):
        g = group(M)

        def fn(host_masks):
            masks = [decoder_dropout_mask(1500, H, 0.5, gen) for _ in range(M)] if host_masks else [dmasks[0]] * M
            g.step([xs[0]] * M, [ys[0]] * M, masks)
        return fn

    if a.prof:
        for _ in range(3):
            group_step(8)(False)
            single_trials(1)(False)
        torch.cuda.synchronize()
        return

    res = {"seed": a.seed, "H": H, "C": C, "O": O, "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "epoch_trials": a.trials, "epoch_frames": int(sum(lengths[1:])), "step_1500_frames": {}, "epoch": {}}
    for M in WIDTHS:
        r = {"single_trials_in_sequence": timed(single_trials(M)), "group_step": timed(group_step(M))}
        for clock in ("device_ms", "wall_ms"):
            r[f"sequence_over_group_{clock[:-3]}"] = r["single_trials_in_sequence"][clock]["median_ms"] / r["group_step"][clock]["median_ms"]
        s, g = r["single_trials_in_sequence"]["device_ms"], r["group_step"]["device_ms"]
        r["device_ranges_overlap"] = not (g["max_ms"] < s["min_ms"] or s["max_ms"] < g["min_ms"])
        res["step_1500_frames"][str(M)] = r
        print(M, json.dumps(r), flush=True)

    # (b) one epoch per model, every model in its own order
    n = a.trials
    ep_len = [lengths[1:]]

    def single_epoch(host_masks):
        g1 = torch.Generator().manual_seed(a.seed + 1)
        for k in torch.randperm(n, generator=g1).tolist():
            m = decoder_dropout_mask(lengths[1 + k], H, 0.5, g1) if host_masks else dmasks[1 + k]
            single._trial(xs[1 + k], ys[1 + k], m, True, 1e-4, 0.99, 1e-8)

    def group_epoch(M):
        g = group(M)

        def fn(host_masks):
            gens = [torch.Generator().manual_seed(a.seed + 1 + m) for m in range(M)]

            def step(trials, masks):
                if not host_masks:
                    masks = [None if k is None else dmasks[1 + k] for k in trials]
                g.step([None if k is None else xs[1 + k] for k in trials], [None if k is None else ys[1 + k] for k in trials], masks)

            _group_epoch(step, gens, [n] * M, ep_len * M, H, 0.5 if host_masks else 0.0, True)
        return fn

    res["epoch"]["single_trainer"] = timed(single_epoch)
    print("epoch single", json.dumps(res["epoch"]["single_trainer"]), flush=True)
    for M in (1, 8):
        r = {"group": timed(group_epoch(M))}
        for clock in ("device_ms", "wall_ms"):
            r[f"M_sequential_epochs_over_group_{clock[:-3]}"] = M * res["epoch"]["single_trainer"][clock]["median_ms"] / r["group"][clock]["median_ms"]
        res["epoch"][str(M)] = r
        print("epoch", M, json.dumps(r), flush=True)
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
