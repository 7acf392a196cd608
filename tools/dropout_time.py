#!/usr/bin/env python3
"""Time the group trainer's step and epoch with the dropout masks drawn on the host (``mask_source="host"``: the CPU generator,
page-locked staging, one upload per step) and on the device (``mask_source="device"``: csrc/dropout.hip, one launch per step), both
in the same session, by the same code.

The shape of tools/decoder_group_time.py: H = 100, C = 64, O = 20, dropout 0.5, float32 frames and targets resident on the device
before the clock starts.  --warmup repetitions, then --reps timed ones; median and min-max.

  --part step --M 8      one ``DecoderGroupTrainerGPU.step`` of M x 1500 frames, both ways.
                         ``wall_ms``: the host's clock from before the masks are drawn until the device is idle.
                         ``device_ms``: between two events; host way: around the step with the masks already resident (the launches
                         alone); device way: around the mask launch and the step.  The device is idle when the first event is
                         recorded, so this interval also holds the host's time to prepare and issue the first launch.
                         ``device_queued_ms``: the same events with one more step (resident masks) enqueued in front of the first
                         event, so that the host runs ahead of the device and the interval holds the device's work alone.
  --part epoch --M 8     one epoch of --trials trials of 250 ... 1500 frames per model, every model in its own shuffled order, both
                         ways: wall clock, and the events around the whole epoch from the same runs.  --steps N times the first N
                         trials per model instead (N steps).
  --part prof            three device-mask steps at M = 1, 8 and 64, for a kernel trace in a run of its own:
                             rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/dropout_time.py --part prof
  --summarize DIR        adds the mask kernel's rows of DIR's kernel stats / trace to the JSON, and the claim's two checks.

Every part is one process and merges its results into profiles/dropout_device.json, so a caller can give every part a time limit
of its own.
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

KERNEL = "dropout_masks_kernel"


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "n": len(ms)}


def load(out):
    return json.load(open(out)) if os.path.exists(out) else {}


def save(out, res):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


def claim(res):
    """The two checks: the wall-clock ranges at M = 8 and 64 do not overlap (device below host), and the step's device time grows
    by no more than the mask kernel's own time (by both device clocks)."""
    out = {}
    for M, r in sorted(res.get("step_1500_frames", {}).items(), key=lambda kv: int(kv[0])):
        h, d = r["host_masks"], r["device_masks"]
        c = {"wall_device_max_below_host_min": d["wall_ms"]["max_ms"] < h["wall_ms"]["min_ms"],
             "wall_host_over_device": h["wall_ms"]["median_ms"] / d["wall_ms"]["median_ms"],
             "device_time_growth_ms": d["device_ms"]["median_ms"] - h["device_ms"]["median_ms"]}
        if "device_queued_ms" in d:
            c["device_queued_time_growth_ms"] = d["device_queued_ms"]["median_ms"] - h["device_queued_ms"]["median_ms"]
        k = res.get("rocprofv3_kernel_trace", {}).get("by_entries", {}).get(M)
        if k:
            c["mask_kernel_ms"] = k["median_us"] / 1e3
            c["growth_within_mask_kernel_time"] = c["device_time_growth_ms"] <= c["mask_kernel_ms"]
            if "device_queued_time_growth_ms" in c:
                c["queued_growth_within_mask_kernel_time"] = c["device_queued_time_growth_ms"] <= c["mask_kernel_ms"]
        out[M] = c
    return out


def summarize(d, out):
    res = load(out)
    prof = {"by_entries": {}}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if KERNEL in row.get("Name", ""):
                prof["stats"] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3,
                                     max_us=float(row["MaxNs"]) / 1e3)
    per = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if KERNEL not in row.get("Kernel_Name", ""):
                continue
            per.setdefault(str(int(row.get("Grid_Size_Y", 0))), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
            for src, dst in (("VGPR_Count", "vgpr"), ("Accum_VGPR_Count", "agpr"), ("SGPR_Count", "sgpr"), ("LDS_Block_Size", "lds_bytes"),
                             ("Scratch_Size", "scratch_bytes")):
                if src in row:
                    prof[dst] = int(row[src])
    for M, us in per.items():                                           # the grid's y extent is the number of entries: M
        prof["by_entries"][M] = {"calls": len(us), "median_us": float(np.median(us)), "min_us": float(np.min(us)), "max_us": float(np.max(us)),
                                 "bytes_stored": int(M) * 1500 * 200 * 4}
        prof["by_entries"][M]["stored_GB_per_s"] = prof["by_entries"][M]["bytes_stored"] / prof["by_entries"][M]["median_us"] / 1e3
    res["rocprofv3_kernel_trace"] = prof
    res["claim"] = claim(res)
    save(out, res)
    print(json.dumps({"rocprofv3_kernel_trace": prof, "claim": res["claim"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("step", "epoch", "prof"), default="step")
    ap.add_argument("--M", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=9500)
    ap.add_argument("--trials", type=int, default=300)
    ap.add_argument("--steps", type=int, default=0, help="epoch part: time the first N trials per model (N steps) instead of all")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_device.json"))
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.out)
    import torch
    import lstm_reference as R
    from dss_amd.training import DecoderGroupTrainerGPU, DeviceMaskSource, _group_epoch, _packed_masks, decoder_dropout_mask

    C, H, O = 64, 100, 20
    sd = R.decoder_state_dict(H, C, 1)
    rng = np.random.default_rng(a.seed)
    n_ep = a.trials if a.part == "epoch" else 0
    lengths = [1500] + rng.integers(250, 1501, a.trials).tolist()[:n_ep]
    xs = [torch.from_numpy(R.frames("x2", 1, n, C, a.seed + k)[0].astype(np.float32)).cuda() for k, n in enumerate(lengths)]
    ys = [torch.from_numpy(rng.standard_normal((n, O)).astype(np.float32)).cuda() for n in lengths]
    gen = torch.Generator().manual_seed(a.seed)
    resident = decoder_dropout_mask(1500, H, 0.5, gen).cuda()

    def timed(fn, clocks, pre=None):
        """fn(clock) runs once per repetition; returns {clock: stats}.  With both clocks asked of one run ("both"), the events and
        the host's clock bracket the same call."""
        out = {}
        for clock in clocks:
            for _ in range(a.warmup):
                fn(clock)
            wall, dev = [], []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if clock == "device_queued_ms":
                    pre()
                t0 = time.perf_counter()
                e0.record()
                fn(clock)
                e1.record()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(e0.elapsed_time(e1))
            if clock in ("wall_ms", "both"):
                out["wall_ms"] = stats(wall)
            if clock in ("device_ms", "device_queued_ms"):
                out[clock] = stats(dev)
            if clock == "both":
                out["events_ms"] = stats(dev)
        return out

    res = load(a.out)
    res.update(seed=a.seed, H=H, C=C, O=O, device=torch.cuda.get_device_name(0), reps=a.reps, warmup=a.warmup)

    for M in a.M:
        g = DecoderGroupTrainerGPU([sd] * M, max_frames=1500)
        sources = [DeviceMaskSource(a.seed + m) for m in range(M)]
        state = {"buf": None}

        if a.part in ("step", "prof"):
            def host_step(clock):
                masks = [decoder_dropout_mask(1500, H, 0.5, gen) for _ in range(M)] if clock == "wall_ms" else [resident] * M
                g.step([xs[0]] * M, [ys[0]] * M, masks)

            def device_step(clock):
                masks, state["buf"] = _packed_masks([(1500, 2 * H, s.seed, s.take(), 0.5) for s in sources], "cuda", state["buf"])
                g.step([xs[0]] * M, [ys[0]] * M, masks)

            if a.part == "prof":
                for _ in range(3):
                    device_step("device_ms")
                torch.cuda.synchronize()
                continue
            clocks, pre = ("device_ms", "device_queued_ms", "wall_ms"), lambda: host_step("device_ms")
            r = {"host_masks": timed(host_step, clocks, pre), "device_masks": timed(device_step, clocks, pre)}
            res.setdefault("step_1500_frames", {})[str(M)] = r
            print("step", M, json.dumps(r), flush=True)
        else:
            n = a.steps or a.trials
            ep_len = [lengths[1:1 + n]]

            def epoch(device):
                def fn(clock):
                    gens = [torch.Generator().manual_seed(a.seed + 1 + m) for m in range(M)]

                    def step(trials, masks):
                        g.step([None if k is None else xs[1 + k] for k in trials], [None if k is None else ys[1 + k] for k in trials], masks)

                    _group_epoch(step, gens, [n] * M, ep_len * M, H, 0.5, True, sources=sources if device else None)
                return fn

            r = {"host_masks": timed(epoch(False), ("both",)), "device_masks": timed(epoch(True), ("both",)),
                 "steps_timed": n, "steps_of_an_epoch": a.trials, "frames_per_model": int(sum(ep_len[0]))}
            r["wall_host_over_device"] = r["host_masks"]["wall_ms"]["median_ms"] / r["device_masks"]["wall_ms"]["median_ms"]
            res.setdefault("epoch", {})[str(M)] = r
            print("epoch", M, json.dumps(r), flush=True)
        del g
    if a.part != "prof":
        res["claim"] = claim(res)
        save(a.out, res)


if __name__ == "__main__":
    main()
