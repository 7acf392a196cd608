"""Development aid: a session's trial list, the only way the streaming API offers (one extract_raw per trial on a sliced copy)
against the one-call host and device paths, and the CPU chain on 1 and 16 cores.

    python tools/session_time.py [--out profiles/session_trials.json] [--reps 20]
    python tools/session_time.py --prof      # only the kernels, for one rocprofv3 --kernel-trace --stats run of its own:
                                             # hga_trials_kernel and hga_fused_kernel on 300 equal-length 2.5 s trials

300 seeded trials of 1.0-4.0 s in a 10-minute 129-column recording; medians and interquartile ranges over the repetitions.
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("delayed-speech-synthesis_amd", "tests", "oracle", os.path.join("oracle", "_ref")):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np

FS, T_REC, C_RAW, N_TRIALS = 1000, 600_000, 129, 300


def workload():
    rng = np.random.default_rng(9000)
    rec = rng.standard_normal((T_REC, C_RAW)) * 50.0
    ranges = []
    for _ in range(N_TRIALS):
        n = int(rng.integers(1000, 4001))
        ranges.append((int(rng.integers(0, T_REC - n)), n))
    return rec, ranges


def stats(ts):
    q1, med, q3 = np.percentile(np.asarray(ts) * 1e3, [25, 50, 75])
    return {"median_ms": round(float(med), 3), "iqr_ms": round(float(q3 - q1), 3), "reps": len(ts)}


def repeat(fn, reps, warm=2):
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return ts


_CPU = {}


def _cpu_setup():
    """The CPU chain: the reference's compiled module + scipy (oracle/make_golden.py RefExtractor) when oracle/_ref is there,
    else this repository's oracle; the pre-transforms are oracle/ecog_chain_oracle.py's restatement in both cases."""
    if _CPU:
        return
    from ecog_chain_oracle import reference_chain
    from dss_amd.hga import reference_filters
    both, car, _ = reference_chain()
    hg, fh, zi_hg, zi_fh = reference_filters(FS)
    ref_so = [f for f in os.listdir(os.path.join(ROOT, "oracle", "_ref")) if f.startswith("hga_optimized")] \
        if os.path.isdir(os.path.join(ROOT, "oracle", "_ref")) else []
    if ref_so:
        import importlib.util
        spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "oracle", "make_golden.py"))
        mg = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mg)
        sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))
        make = lambda: mg.RefExtractor(FS, 128, hg, fh, zi_hg, zi_fh)
        _CPU["chain"] = "reference hga_optimized + scipy.signal.sosfilt"
    else:
        import oracle_api
        orc = oracle_api.Oracle(os.path.join(ROOT, "oracle", "liboracle.so"))
        make = lambda: orc.extractor({"sos_hg": hg, "sos_fh": fh, "zi_hg": zi_hg, "zi_fh": zi_fh}, 128)
        _CPU["chain"] = "oracle/liboracle.so"
    _CPU["run"] = lambda chunk: make().extract(car(both(chunk)))


def _cpu_trial(args):
    _cpu_setup()
    rec, (s, n) = args
    return _CPU["run"](rec[s:s + n]).shape[0]


def cpu_chain(rec, ranges, procs):
    import multiprocessing as mp
    _cpu_setup()
    t = time.perf_counter()
    if procs == 1:
        n = sum(_cpu_trial((rec, r)) for r in ranges)
    else:
        global _REC
        _REC = rec
        with mp.get_context("fork").Pool(procs) as pool:
            n = sum(pool.map(_cpu_pooled, ranges, chunksize=4))
    return time.perf_counter() - t, n


def _cpu_pooled(r):
    return _cpu_trial((_REC, r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_trials.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--prof", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    rec, ranges = workload()
    res = {"workload": f"{N_TRIALS} trials of 1.0-4.0 s in a {T_REC // FS} s x {C_RAW}-column recording, 128 output channels",
           "stream_seconds": round(sum(n for _, n in ranges) / FS, 3)}
    if not a.prof and not a.no_cpu:          # before the GPU is opened: the pool forks
        t1, n1 = cpu_chain(rec, ranges, 1)
        t16, n16 = cpu_chain(rec, ranges, 16)
        assert n1 == n16
        res["cpu_chain"] = {"chain": _CPU["chain"], "one_core_s": round(t1, 3), "sixteen_processes_s": round(t16, 3), "reps": 1}
        print(res["cpu_chain"], flush=True)
    import torch
    from dss_amd import session
    from dss_amd.hga import HgaExtractorGPU
    if a.prof:
        n = 2500
        eq = [(i * 1900, n) for i in range(N_TRIALS)]
        ex = session.session_extractor(C_RAW, FS)
        d_rec = torch.from_numpy(rec).cuda()
        for _ in range(5):
            ex.extract_trials_torch(d_rec, eq)
            ex.extract_trials_torch(d_rec, ranges)
        st = HgaExtractorGPU(N_TRIALS, 128, fs=FS)
        x = torch.from_numpy(np.random.default_rng(1).standard_normal((N_TRIALS, n, 128)) * 50.0).cuda()
        for _ in range(5):
            st.reset()
            st.extract_torch(x)
        torch.cuda.synchronize()
        print("prof run done: %d equal trials of %d rows = %.1f stream-s per launch; ragged list %.1f stream-s"
              % (N_TRIALS, n, N_TRIALS * n / FS, res["stream_seconds"]))
        return
    old = HgaExtractorGPU(1, 128, fs=FS)
    old.set_frontend(C_RAW, *session.offline_frontend())

    def per_trial():
        out = []
        for s, n in ranges:
            old.reset()
            out.append(old.extract_raw(rec[s:s + n].copy())[0])
        return np.concatenate(out)

    ex = session.session_extractor(C_RAW, FS)
    want = per_trial()
    assert np.array_equal(ex.extract_trials(rec, ranges), want)
    res["frames"] = int(len(want))
    res["per_trial_extract_raw"] = stats(repeat(per_trial, a.reps, warm=1))
    print("per trial", res["per_trial_extract_raw"], flush=True)
    res["one_call_host"] = stats(repeat(lambda: ex.extract_trials(rec, ranges), a.reps))
    print("one call host", res["one_call_host"], flush=True)
    d_rec = torch.from_numpy(rec).cuda()
    res["one_call_device_resident"] = stats(repeat(lambda: ex.extract_trials_torch(d_rec, ranges), a.reps))
    print("one call device", res["one_call_device_resident"], flush=True)
    res["one_call_device_with_upload"] = stats(repeat(lambda: ex.extract_trials_torch(torch.from_numpy(rec).cuda(), ranges).cpu(), a.reps))
    print("one call device incl. H2D of the recording and D2H of the frames", res["one_call_device_with_upload"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
