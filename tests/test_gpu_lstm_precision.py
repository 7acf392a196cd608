"""The two LSTM kernels against a float64 restatement of their models (tests/lstm_reference.py), not against a float32 peer.

csrc/bilstm_decoder.hip (BiLstmDecoderGPU, dss_dec_forward_dev / dss_dec_forward_rows_dev) and csrc/vad_lstm.hip (VadLstmGPU,
dss_vad_step_dev) compute in float32 with fused multiply-adds, so their parity grade is a tolerance.  Here it is held against
float64: outputs (features, logits) and h within an absolute lstm_reference.bound(scale) -- 2e-6 for default-init weights,
5e-5 for the LSTM weights x4, whose measured reason is given there -- c within lstm_reference.C_REL of max(|c|, 1).  Every test prints, beside the kernel's largest error, torch.nn.LSTM's in float32 on the same GPU (run with -rP
to see them).  The bound is what float32 arithmetic leaves; the power checks in tests/test_cpu_lstm_reference.py show that a
kernel with one wrong weight, one missing bias term or one misread chunk tail misses it by 10x on these same inputs.
The float64 reference runs on a fixed subset of the streams when S is large (lstm_reference.sample_streams)."""
import numpy as np
import pytest
import torch

import lstm_reference as R

pytestmark = pytest.mark.gpu

torch.set_num_threads(min(torch.get_num_threads(), 16))


def _err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max()) if np.size(want) else 0.0


def _c_err(got, want):
    """|c - c_ref| / max(|c_ref|, 1), the largest."""
    return float((np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), 1.0)).max())


def _torch_module(cls, sd, H, C):
    m = cls(nb_layer=2, nb_hidden_units=H, nb_electrodes=C).eval()
    m.load_state_dict(sd)
    return m.cuda()


def _report(name, **errs):
    print(f"{name}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("H,C", [(100, 64), (7, 5), (33, 17), (128, 256)])
def test_decoder_plain_against_float64(H, C, scale):
    """dss_dec_forward_dev from the zero state: every case of lstm_reference.decoder_cases (T 1 ... 2000, S 1 ... 1024 so W = 1,
    2, 4, x2 / x30 / constant / zero frames, float32 and float64 frames), features within the bound of float64."""
    from dss_amd.decoder import BiLstmDecoderGPU
    from dss_amd.models import BidirectionalSpeechSynthesisModel
    sd = R.decoder_state_dict(H, C, scale)
    net = R.Net(sd)
    mg = _torch_module(BidirectionalSpeechSynthesisModel, sd, H, C)
    cases = R.decoder_cases(H, C)
    worst_k, worst_t, fails = 0.0, 0.0, []
    for S, T, kind, f64, seed in cases:
        x = R.frames(kind, S, T, C, seed)
        xd = torch.from_numpy(x if f64 else x.astype(np.float32)).cuda()
        got = BiLstmDecoderGPU(S, T, state_dict=sd)(xd)
        pick = R.sample_streams(S)
        want, _ = R.decoder_forward(net, x[pick])
        with torch.no_grad():
            tw, _ = mg(xd[pick].float(), mg.create_new_initial_state(batch_size=len(pick), device="cuda"))
        ek, et = _err(got[pick].cpu().numpy(), want), _err(tw.cpu().numpy(), want)
        worst_k, worst_t = max(worst_k, ek), max(worst_t, et)
        if not ek <= R.bound(scale):
            fails.append((S, T, kind, f64, ek, et))
    _report(f"decoder H={H} C={C} x{scale}", kernel=worst_k, torch_fp32=worst_t)
    assert not fails, f"|features - float64| > {R.bound(scale)} (S, T, kind, f64, kernel, torch): {fails}"


@pytest.mark.parametrize("scale", [1, 4])
def test_decoder_ragged_against_float64(scale):
    """dss_dec_forward_rows_dev, 257 segments so that workgroups carry W = 4: the first workgroup holds lengths 2000, 1, 0 and 777,
    the rest short ones, read from scattered rows of a pool with 2100 frames per row.  Each segment within the bound of the float64
    decoder run on that segment alone (its backward direction starts at its own last frame); nothing written past a length."""
    from dss_amd.decoder import BiLstmDecoderGPU
    from dss_amd.models import BidirectionalSpeechSynthesisModel
    H, C, T = 100, 64, 2000
    sd = R.decoder_state_dict(H, C, scale)
    net = R.Net(sd)
    mg = _torch_module(BidirectionalSpeechSynthesisModel, sd, H, C)
    counts, rows, pool = R.ragged_case(scale)
    n = len(counts)
    k = BiLstmDecoderGPU(n, T, state_dict=sd)
    feats = torch.full((n, T, 20), 777.0, dtype=torch.float32, device="cuda")
    k.forward_rows_torch(torch.from_numpy(pool.astype(np.float32)).cuda(), rows, counts, feats, T)
    got = feats.cpu().numpy()
    worst_k, worst_t, fails = 0.0, 0.0, []
    for i in R.sample_streams(n):
        L = int(counts[i])
        assert (got[i, L:] == 777.0).all(), f"segment {i} ({L} frames): features written past its length"
        if not L:
            continue
        seg = pool[rows[i], :L][None]
        want, _ = R.decoder_forward(net, seg)
        with torch.no_grad():
            tw, _ = mg(torch.from_numpy(seg).float().cuda(), mg.create_new_initial_state(batch_size=1, device="cuda"))
        ek, et = _err(got[i, :L], want[0]), _err(tw[0].cpu().numpy(), want[0])
        worst_k, worst_t = max(worst_k, ek), max(worst_t, et)
        if not ek <= R.bound(scale):
            fails.append((i, L, ek, et))
    _report(f"decoder ragged x{scale}", kernel=worst_k, torch_fp32=worst_t)
    assert not fails, f"|features - float64| > {R.bound(scale)} (segment, frames, kernel, torch): {fails}"
    assert all((got[i, int(counts[i]):] == 777.0).all() for i in range(n))


def _vad_run(name, H, C, S, scale, kind, sizes, seed, pick, reset_at=None, reset_stream=None):
    """Steps VadLstmGPU(S) packet by packet through the frames, torch.nn.LSTM (float32, GPU) and the float64 reference (streams
    `pick` only) alongside, all carrying state; at frame `reset_at` stream `reset_stream` is reset in all three.  Returns a dict
    of the largest errors of each against float64 and the label statistics; asserts the bounds."""
    from dss_amd.models import UnidirectionalVoiceActivityDetector
    from dss_amd.vad import VadLstmGPU
    sd = R.vad_state_dict(H, C, scale)
    net = R.Net(sd)
    mg = _torch_module(UnidirectionalVoiceActivityDetector, sd, H, C)
    k = VadLstmGPU(S, state_dict=sd)
    n = sum(sizes)
    x = R.frames(kind, S, n, C, seed)
    xd = torch.from_numpy(x.astype(np.float32)).cuda()
    pi = torch.as_tensor(pick, device="cuda")
    state = None
    tstate = mg.create_new_initial_state(batch_size=len(pick), device="cuda")
    logits, labels, want, twant = [], [], [], []
    j = pick.index(reset_stream) if reset_stream is not None else None
    t0 = 0
    for w in sizes:
        if t0 == reset_at:
            k.reset(reset_stream)
            for a in state:
                a[:, j] = 0.0
            tstate = (tstate[0].clone(), tstate[1].clone())
            tstate[0][:, j] = 0.0
            tstate[1][:, j] = 0.0
        lab, lg = k.step_torch(xd[:, t0:t0 + w] if w % 2 else xd[:, t0:t0 + w].double(), want_logits=True)
        logits.append(lg[pi])
        labels.append(lab[pi])
        ref, state = R.vad_forward(net, x[pick, t0:t0 + w], state)
        want.append(ref)
        with torch.no_grad():
            tw, tstate = mg(xd[pi, t0:t0 + w], tstate)
        twant.append(tw)
        t0 += w
    logits = torch.cat(logits, 1).cpu().numpy()
    labels = torch.cat(labels, 1).cpu().numpy()
    want = np.concatenate(want, 1)
    twant = torch.cat(twant, 1).cpu().numpy()
    h, c = k.state()
    h, c = h[:, pick], c[:, pick]
    r = dict(logits=_err(logits, want), torch_logits=_err(twant, want), h=_err(h, state[0]),
             torch_h=_err(tstate[0].cpu().numpy(), state[0]), c_rel=_c_err(c, state[1]),
             torch_c_rel=_c_err(tstate[1].cpu().numpy(), state[1]), max_abs_c=float(np.abs(state[1]).max()))
    margin = want[..., 1] - want[..., 0]
    sure = np.abs(margin) > 2 * R.bound(scale)
    r["near_ties"] = int((~sure).sum())
    r["label_diffs"] = int((labels[sure] != (margin[sure] > 0)).sum())
    _report(name, **r)
    assert r["logits"] <= R.bound(scale) and r["h"] <= R.bound(scale) and r["c_rel"] <= R.C_REL, r
    assert r["label_diffs"] == 0, r
    return r


R_RESET_AT = sum(R.vad_packets(6000, 6)[:750])            # a packet boundary near the middle


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("kind", ["x2", "x30"])
def test_vad_long_carry_against_float64(kind, scale):
    """16 streams x 6000 frames (a minute of frames) in packets of 4 with occasional 1s and 5s, state carried by the kernel from
    packet to packet; stream 5 is reset at frame 3000 (the float64 reference zeroes that stream's state there).  Logits, h, c
    within the bounds at every frame / at the end; labels equal the float64 argmax wherever its margin exceeds 2 x the bound."""
    S = 16
    _vad_run(f"vad 16x6000 {kind} x{scale}", 150, 64, S, scale, kind, R.vad_packets(6000, 6), 70, list(range(S)),
             reset_at=R_RESET_AT, reset_stream=5)



@pytest.mark.parametrize("scale", [1, 4])
def test_vad_128_streams_1000_frames_against_float64(scale):
    """128 streams x 1000 frames (one stream per workgroup), the float64 reference on a subset of the streams."""
    _vad_run(f"vad 128x1000 x{scale}", 150, 64, 128, scale, "x2", R.vad_packets(1000, 8), 80, R.sample_streams(128))


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("H,C", [(150, 64), (160, 128)])
@pytest.mark.parametrize("S", [256, 257, 513])
def test_vad_many_streams_against_float64(S, H, C, scale):
    """256 streams (SW = 1), 257 and 513 (SW = 2, the last workgroup half empty), at the reference's size and at the kernel's
    largest, 60 frames in packets of 4, 1 and 5."""
    _vad_run(f"vad S={S} H={H} C={C} x{scale}", H, C, S, scale, "x2", R.vad_packets(60, S), 90 + S, R.sample_streams(S))
