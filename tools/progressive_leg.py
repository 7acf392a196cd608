"""Progressive segment delivery (SegmentSynthesisQueue(progressive=True)) against the whole-segment path, in one process:

    python tools/progressive_leg.py [--out FILE]      ->  one JSON object (profiles/progressive_leg.json)

(a) The paced 128-stream gated pass of tools/gated_leg.py (same input, same detector, 40 ms cadence, the host polling between
    ticks) once with progressive=False and once with progressive=True: tick p50 / p99 / max, segment close -> first PCM on the
    host, the lane-wait and launch -> first PCM shares of it, and close -> last PCM.  Without the option the first PCM of a
    segment is its whole PCM.
(b) The sample-rate kernel alone, ragged against progressive: 32 rows x 350 frames from identical (fresh) slot states, the two
    forms alternated, 5 repeats each, dss_lpcnet_batch_kernel_ms per call."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "delayed-speech-synthesis_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
FRAME = 160


def paced(packets, progressive):
    import gc
    import numpy as np
    import gated_leg
    from dss_amd.pipeline import GatedStreamingPipeline
    pct = lambda a, q: float(np.percentile(a, q)) if len(a) else None
    gp = GatedStreamingPipeline(gated_leg.S, 64, channel_means=np.full(64, 5.0), vad=gated_leg.detector(), max_segment_frames=1040,
                                progressive=progressive)
    q = gp.queue
    tick_ms, n_seg, n_chunks = [], 0, 0

    def poll():
        nonlocal n_seg, n_chunks
        n_seg += len(gp.poll())
        if progressive:
            n_chunks += len(gp.poll_chunks())
    gc.collect()
    gc.disable()
    t_start = time.perf_counter()
    for k in range(gated_leg.TICKS):
        due = t_start + 0.04 * k                                 # the amplifier's cadence; the host polls while it waits
        while True:
            left = due - time.perf_counter()
            if left <= 0:
                break
            poll()
            if left > 0.002:
                time.sleep(0.0005)
        if k == gated_leg.WARM:
            for d in (q.latencies_ms, q.first_pcm_latencies_ms, q.lane_wait_ms, q.launch_to_first_pcm_ms):
                d.clear()
            n_seg = n_chunks = 0
        t0 = time.perf_counter()
        n_seg += len(gp.push(packets[k]))
        ms = (time.perf_counter() - t0) * 1e3
        if k >= gated_leg.WARM:
            tick_ms.append(ms)
    while q.in_flight:
        poll()
        time.sleep(0.0005)
    poll()
    gc.enable()
    last = list(q.latencies_ms)
    first = list(q.first_pcm_latencies_ms) if progressive else last
    res = {"progressive": progressive, "ticks": len(tick_ms), "tick_p50_ms": pct(tick_ms, 50), "tick_p99_ms": pct(tick_ms, 99),
           "tick_max_ms": max(tick_ms), "segments": n_seg, "chunks": n_chunks if progressive else None,
           "close_to_first_pcm_p50_ms": pct(first, 50), "close_to_first_pcm_p99_ms": pct(first, 99),
           "lane_wait_p50_ms": pct(q.lane_wait_ms, 50), "lane_wait_p99_ms": pct(q.lane_wait_ms, 99),
           "launch_to_first_pcm_p50_ms": pct(q.launch_to_first_pcm_ms, 50) if progressive else None,
           "launch_to_first_pcm_p99_ms": pct(q.launch_to_first_pcm_ms, 99) if progressive else None,
           "close_to_last_pcm_p50_ms": pct(last, 50), "close_to_last_pcm_p99_ms": pct(last, 99), "lanes": len(q.lanes)}
    gp.close()
    del gp
    return res


def kernel_ab(rows=32, frames=350, repeats=5):
    import ctypes as C
    import numpy as np
    import torch
    from dss_amd import _lib
    from dss_amd.lpcnet import LPCNetBatch
    from dss_amd.lpcnet_weights import synthetic_features
    L = _lib.load()
    b = LPCNetBatch(rows, frames)
    b.set_multi(1)                                               # the progressive call's kernel for both forms
    feats = torch.from_numpy(np.stack([synthetic_features(1000 + r, frames) for r in range(rows)])).cuda()
    counts, slots = [frames] * rows, list(range(rows))
    host = L.dss_host_alloc_fine(rows * frames * FRAME * 2)
    done = L.dss_host_alloc_fine(rows * 4)
    assert host and done, L.dss_last_error().decode()
    ms = {"ragged": [], "progressive": []}
    try:
        for rep in range(repeats + 1):                           # the first round warms both up and is not kept
            for form in ("ragged", "progressive"):
                b.reset()                                        # identical slot states for every call
                b.enable_timing(True)
                if form == "ragged":
                    b.synthesize_ragged_torch(feats, counts, slots=slots)
                else:
                    b.synthesize_ragged_progress_torch(feats, counts, slots, host, done)
                torch.cuda.synchronize()
                if rep:
                    ms[form].append(b.kernel_ms(0))
                b.enable_timing(False)
        got = np.ctypeslib.as_array((C.c_int16 * (rows * frames * FRAME)).from_address(host)).reshape(rows, -1).copy()
        b.reset()
        want = b.synthesize_ragged_torch(feats, counts, slots=slots).cpu().numpy()
        same = bool(np.array_equal(got, want))
    finally:
        torch.cuda.synchronize()
        L.dss_host_free(host)
        L.dss_host_free(done)
    per = {f: [v / frames * 1e3 for v in x] for f, x in ms.items()}       # microseconds per frame
    mr, mp = float(np.median(ms["ragged"])), float(np.median(ms["progressive"]))
    return {"rows": rows, "frames": frames, "repeats": repeats, "sample_kernel_ms": ms, "us_per_frame": per,
            "median_ms": {"ragged": mr, "progressive": mp}, "progressive_over_ragged": mp / mr,
            "spread_ragged": (max(ms["ragged"]) - min(ms["ragged"])) / mr, "pcm_bit_identical": same}


def leg():
    import gated_leg
    packets = gated_leg.make_input()
    out = {"config": "tools/gated_leg.py's paced 128-stream pass (seeded detector, loud / quiet synthetic input, 40 ms cadence, host "
                     "polling every 0.5 ms between ticks) with the whole-segment queue and with progressive=True; then the sample "
                     "kernel alone, ragged against progressive",
           "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES")}
    out["paced_40ms_whole_segment"] = paced(packets, False)
    out["paced_40ms_progressive"] = paced(packets, True)
    out["kernel_ab"] = kernel_ab()
    return out


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--hw-queues", type=int, default=8)
    a = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", str(a.hw_queues))
    os.environ.setdefault("DSS_LPCNET_SYNTHETIC", "1")
    res = leg()
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
