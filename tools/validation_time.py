#!/usr/bin/env python3
"""Time the validation passes of the two recurrent models over a synthetic corpus: 300 trials of 250 ... 1500 frames (drawn with
--seed), 64 channels, N(0, 1) x 2 frames (tests/lstm_reference.frames), H = 150 detector and H = 100 decoder at default init.

  detector: (i) one ``vad_validation`` call, from a state_dict (handle created inside) and with a handle the caller keeps; (ii) what there was before it: per trial ``reset`` + ``step_torch`` on a one-stream
            handle, scored in numpy on the host; (iii) the torch module per trial on the same GPU, scored with torch.
  decoder:  (i) one ``decoder_validation`` call, both ways; (ii) per trial ``forward_rows_torch`` (one segment), MSE in numpy; (iii) the torch
            module per trial, nn.MSELoss.

Host arrays in, host scores out, wall clock with the device idle before and after; --reps repetitions after --warmup, median
and min-max; writes profiles/validation_trials.json.

    python tools/validation_time.py [--reps 5] [--warmup 1] [--seed 9300]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=9300)
    ap.add_argument("--trials", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validation_trials.json"))
    a = ap.parse_args()
    import torch
    import lstm_reference as R
    from dss_amd.decoder import BiLstmDecoderGPU
    from dss_amd.models import BidirectionalSpeechSynthesisModel, UnidirectionalVoiceActivityDetector
    from dss_amd.vad import VadLstmGPU
    from dss_amd.validation import decoder_validation, trial_bounds, vad_validation

    C = 64
    rng = np.random.default_rng(a.seed)
    lengths = rng.integers(250, 1501, a.trials)
    n = int(lengths.sum())
    x = R.frames("x2", 1, n, C, a.seed + 1)[0]
    ids = np.concatenate([np.full(m, (k % 9 + 1) * (-1) ** k, np.int16) for k, m in enumerate(lengths)])
    labels = np.repeat(rng.integers(0, 2, n // 25 + 1), 25)[:n].astype(bool)
    lpc = rng.standard_normal((n, 20)).astype(np.float32)
    ranges = trial_bounds(ids)
    assert [m for _, m in ranges] == lengths.tolist()
    vsd, dsd = R.vad_state_dict(150, C, 1), R.decoder_state_dict(100, C, 1)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return stats(ms)

    # ---- detector
    one = VadLstmGPU(1, state_dict=vsd)

    def vad_loop():
        xd = torch.from_numpy(x).cuda()
        loss, correct = 0.0, 0
        for first, m in ranges:
            one.reset()
            lab, lg = one.step_torch(xd[None, first:first + m], want_logits=True)
            z, lab = lg[0].cpu().numpy().astype(np.float64), lab[0].cpu().numpy()
            t = labels[first:first + m]
            mx = z.max(axis=1)
            loss += float(np.mean(mx + np.log(np.exp(z[:, 0] - mx) + np.exp(z[:, 1] - mx)) - z[np.arange(m), t.astype(np.int64)]))
            correct += int((lab == t).sum())
        return loss, correct / n

    vm = UnidirectionalVoiceActivityDetector(nb_layer=2, nb_hidden_units=150, nb_electrodes=C).eval()
    vm.load_state_dict(vsd)
    vm = vm.cuda()
    cfunc = torch.nn.CrossEntropyLoss()

    def vad_torch():
        xd = torch.from_numpy(x).cuda().float()
        yd = torch.from_numpy(labels).cuda().long()
        loss, correct = 0.0, 0
        with torch.no_grad():
            for first, m in ranges:
                out, _ = vm(xd[None, first:first + m], vm.create_new_initial_state(batch_size=1, device="cuda"))
                loss += cfunc(out.reshape(-1, 2), yd[first:first + m]).item()
                correct += int((out[0].argmax(dim=1) == yd[first:first + m]).sum().item())
        return loss, correct / n

    res = {"seed": a.seed, "trials": int(a.trials), "frames": n, "channels": C, "lengths": [int(lengths.min()), int(lengths.max())],
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup}
    r = vad_validation(vsd, x, labels, ids)
    l2, a2 = vad_loop()
    l3, a3 = vad_torch()
    res["vad"] = {"loss": [r["loss"], l2, l3], "accuracy": [r["accuracy"], a2, a3],
                  "one_call": timed(lambda: vad_validation(vsd, x, labels, ids)),
                  "one_call_kept_handle": timed(lambda: vad_validation(one, x, labels, ids)),
                  "per_trial_step_loop": timed(vad_loop), "torch_module_per_trial": timed(vad_torch)}

    # ---- decoder
    seg = BiLstmDecoderGPU(1, int(lengths.max()), state_dict=dsd)

    def dec_loop():
        xd = torch.from_numpy(x).cuda()
        total = 0.0
        for first, m in ranges:
            feats = torch.empty((1, m, 20), dtype=torch.float32, device="cuda")
            seg.forward_rows_torch(xd[None, first:first + m], None, [m], feats, m)
            d = feats[0].cpu().numpy().astype(np.float64) - lpc[first:first + m]
            total += float(np.mean(d * d))
        return total / len(ranges)

    dm = BidirectionalSpeechSynthesisModel(nb_layer=2, nb_hidden_units=100, nb_electrodes=C).eval()
    dm.load_state_dict(dsd)
    dm = dm.cuda()
    mfunc = torch.nn.MSELoss()

    def dec_torch():
        xd = torch.from_numpy(x).cuda().float()
        yd = torch.from_numpy(lpc).cuda()
        total = 0.0
        with torch.no_grad():
            for first, m in ranges:
                out, _ = dm(xd[None, first:first + m], dm.create_new_initial_state(batch_size=1, device="cuda"))
                total += mfunc(out, yd[None, first:first + m]).item()
        return total / len(ranges)

    r = decoder_validation(dsd, x, lpc, ids)
    kept = BiLstmDecoderGPU(256, int(lengths.max()), state_dict=dsd)
    res["decoder"] = {"loss": [r["loss"], dec_loop(), dec_torch()],
                      "one_call": timed(lambda: decoder_validation(dsd, x, lpc, ids)),
                      "one_call_kept_handle": timed(lambda: decoder_validation(kept, x, lpc, ids)),
                      "per_trial_forward_loop": timed(dec_loop), "torch_module_per_trial": timed(dec_torch)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
