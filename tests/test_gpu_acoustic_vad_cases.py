"""The acoustic VAD kernels (csrc/acoustic_vad.hip) at the shapes of tests/acoustic_vad_cases.py: sampling rates, windows, shifts
and band counts other than 16 kHz / 800 / 160 / 40 against what the reference's own EnergyBasedVad gave there
(tests/golden/acoustic_vad_cases.npz), trial shapes on the 32-frame tile, on the shift, on the lead and on the ends of the audio
against the float64 restatement, the vote bit for bit against dss_avad_vote_host on the kernel's own energies, and two
invariances that hold by the energy kernel's construction.  tests/test_cpu_acoustic_vad_cases.py proves without a device that
every case reaches the branch it names and that the bounds come from the CPU alone.

Labels are compared on EVERY frame: no frame of the fixture or of the edge trials lies within GAP = 1e-6 of its trial's
threshold (asserted by the generator and by the CPU test), and no bound on the log energy passes 1e-10.  Frames compared: 1507
of the geometry cases against the fixture, 515 of the edge trials against the restatement, none left out.

The kernel's worst deviation from the fixture is printed per case; the figures of an MI355X stand beside the bounds in
``acoustic_vad_cases.KERNEL_MEASURED``."""
import numpy as np
import pytest

import acoustic_vad_cases as vc
import acoustic_vad_reference as ref

pytestmark = pytest.mark.gpu


def _vad(**kw):
    from dss_amd.acoustic_vad import AcousticVadGPU
    return AcousticVadGPU(**kw)


def _case_vad(c):
    v = _vad(fs=c.fs, window_length=c.window_length, frame_shift=c.frame_shift, n_bands=c.n_bands)
    assert (v.window, v.shift, v.n_bins) == (c.N, c.shift, c.bins)
    return v


def _vote_is_the_hosts(labels, le, thr, counts, **params):
    """dss_avad_vote_host on the kernel's own energies: the kernel's threshold bit for bit, its labels on every frame."""
    from dss_amd.acoustic_vad import vote_host
    pos = 0
    for k, W in enumerate(counts):
        want, want_thr = vote_host(le[pos:pos + W], **params)
        assert want_thr == thr[k], (k, W, want_thr, thr[k])
        assert np.array_equal(want, labels[pos:pos + W]), (k, W)
        pos += W
    assert pos == len(labels) == len(le)


@pytest.fixture(scope="module")
def cases_fixture(golden):
    g = golden("acoustic_vad_cases.npz")
    assert tuple(str(n) for n in g["names"]) == vc.NAMES
    return g


@pytest.mark.parametrize("name", vc.NAMES)
def test_geometry_against_the_reference(cases_fixture, name):
    import torch
    g, c, k = cases_fixture, vc.case(name), vc.NAMES.index(name)
    b = np.concatenate([[0], np.cumsum(g["frame_counts"])])
    a, z = b[4 * k], b[4 * k + 4]
    wav, trials = vc.audio(name), vc.trials(name)
    v = _case_vad(c)
    try:
        labels, le, thr = v.labels_trials(wav, trials, return_energy=True)
        assert labels.shape == le.shape == (z - a,) and thr.shape == (4,)
        worst = float(np.max(np.abs(le - g["log_energy"][a:z])))
        worst_thr = float(np.max(np.abs(thr - g["thresholds"][4 * k:4 * k + 4])))
        print(f"{name}: kernel vs reference over {z - a} frames, max |log energy difference| {worst:.3e}, threshold {worst_thr:.3e}, "
              f"bound {vc.bound(name):.3e} (D {c.D:.3e}, U {vc.U[name]:.3e})")
        assert vc.bound(name) <= vc.CAP
        assert np.array_equal(labels, g["labels"][a:z])                                  # every frame, none left out
        assert worst <= vc.bound(name)
        assert worst_thr <= vc.bound(name)
        _vote_is_the_hosts(labels, le, thr, vc.TRIAL_FRAMES)
        assert np.array_equal(v.labels_trials(wav, trials), labels)                      # the plain form
        # the device-resident form gives the host form's bits
        d_lab, d_le, d_thr = v.labels_trials_torch(torch.from_numpy(wav.copy()).cuda(), trials, return_energy=True)
        torch.cuda.synchronize()
        assert np.array_equal(d_lab.cpu().numpy().astype(bool), labels)
        assert np.array_equal(d_le.cpu().numpy(), le) and np.array_equal(d_thr.cpu().numpy(), thr)
        # and a trial alone has the bits it has in the list
        for j, t in enumerate(trials):
            lab1, le1, thr1 = v.labels_trials(wav, [t], return_energy=True)
            assert np.array_equal(le1, le[b[4 * k + j] - a:b[4 * k + j + 1] - a]) and thr1[0] == thr[j], (name, j)
            assert np.array_equal(lab1, labels[b[4 * k + j] - a:b[4 * k + j + 1] - a]), (name, j)
    finally:
        v.close()


@pytest.fixture(scope="module")
def default_vad():
    v = _vad()
    yield v
    v.close()


def _edge_call(v, which, device=False):
    """All edge trials of one audio in one list -> (edges, labels, log energies, thresholds)."""
    es = vc.edges(which)
    wav = vc.edge_audio(which)
    ranges, lead = [(e.first, e.length) for e in es], [e.lead for e in es]
    if not device:
        return es, v.labels_trials(wav, ranges, lead=lead, return_energy=True)
    import torch
    d = torch.from_numpy(wav.copy()).cuda()
    assert d.shape[0] == len(wav)                                # exactly the audio: nothing behind its last sample
    out = v.labels_trials_torch(d, ranges, lead=lead, return_energy=True)
    torch.cuda.synchronize()
    return es, (out[0].cpu().numpy().astype(bool), out[1].cpu().numpy(), out[2].cpu().numpy())


@pytest.mark.parametrize("which", ["speech", "noise"])
def test_trial_edges_against_the_restatement(default_vad, which):
    v = default_vad
    wav = vc.edge_audio(which)
    es, (labels, le, thr) = _edge_call(v, which)
    pos, worst = 0, 0.0
    for k, e in enumerate(es):
        want_le = ref.log_energy(ref.trial_samples(wav, e.first, e.length, e.lead), v.window_fn, v.mel)
        assert len(want_le) == e.W
        dev = float(np.max(np.abs(le[pos:pos + e.W] - want_le)))
        worst = max(worst, dev)
        assert dev <= vc.LOG_ENERGY_BOUND, (e.name, dev)
        want, want_thr, gap = ref.vote(want_le)
        assert gap >= vc.GAP, e.name
        assert abs(thr[k] - want_thr) <= vc.LOG_ENERGY_BOUND + 1e-12 * abs(want_thr), e.name
        assert np.array_equal(labels[pos:pos + e.W], want), e.name                     # every frame
        pos += e.W
    assert pos == len(labels)
    print(f"edges ({which}): {pos} frames, kernel vs restatement max |log energy difference| {worst:.3e}, bound {vc.LOG_ENERGY_BOUND:.3e}")
    _vote_is_the_hosts(labels, le, thr, [e.W for e in es])
    # the device-resident form, on a tensor of exactly the audio's samples, and every trial alone: the same bits
    _, dev_out = _edge_call(v, which, device=True)
    assert np.array_equal(dev_out[0], labels) and np.array_equal(dev_out[1], le) and np.array_equal(dev_out[2], thr)
    pos = 0
    for k, e in enumerate(es):
        lab1, le1, thr1 = v.labels_trials(wav, [(e.first, e.length)], lead=e.lead, return_energy=True)
        assert np.array_equal(le1, le[pos:pos + e.W]) and thr1[0] == thr[k] and np.array_equal(lab1, labels[pos:pos + e.W]), e.name
        pos += e.W
    if which == "speech":
        by = {e.name: k for k, e in enumerate(es)}
        starts = np.concatenate([[0], np.cumsum([e.W for e in es])])
        a, b = by["twice_a"], by["twice_b"]
        assert not np.array_equal(le[starts[a]:starts[a + 1]], le[starts[b]:starts[b + 1]])    # the same range, another lead
        k = by["lead_whole_at_end"]
        assert np.all(le[starts[k]:starts[k + 1]] == le[starts[by["lead_whole"]]]) and not labels[starts[k]:starts[k + 1]].any()


@pytest.mark.parametrize("mean_scale", vc.VOTE_MEAN_SCALES)
@pytest.mark.parametrize("context", vc.VOTE_CONTEXTS)
def test_vote_is_the_host_functions_bit_for_bit(context, mean_scale):
    """avad_vote_kernel sums in dss_avad_vote_host's order (256 strided sums, a halving tree): on the kernel's own energies the
    two agree bit for bit, with nothing left out, at 1 .. 700 frames and around the 256 strided sums."""
    wav, trials = vc.vote_audio(), vc.vote_trials()
    # the list's log energies lie between -431 and -231 with means around -380: both constants put the thresholds inside that
    # range, so that both labels occur (the restatement gives 0 to 10 of 10 and about 190 of 700)
    params = dict(frames_context=context, energy_mean_scale=mean_scale, energy_threshold=590.0 if mean_scale else -380.0)
    v = _vad(**params)
    try:
        labels, le, thr = v.labels_trials(wav, trials, return_energy=True)
        _vote_is_the_hosts(labels, le, thr, vc.VOTE_FRAMES, **params)
        if mean_scale == 0.0:
            assert np.all(thr == -380.0)
        if context:
            assert labels.any() and not labels.all()
        else:
            assert labels.all()                                  # an empty window: 0 >= 0 * proportion
    finally:
        v.close()


@pytest.mark.parametrize("name", vc.INVARIANCE_CASES)
def test_exact_invariances(name):
    """Every output element of avad_energy_kernel accumulates over k in the same order whatever its row, its tile or its trial.
    (a) A trial with lead = L has the bits of the same samples with the L zeros written into the audio and lead = 0.
    (b) Frame f of a 71-frame trial has the bits of frame 0 of the one-window trial that starts f shifts later."""
    kw, N, shift, wav = vc.invariance_case(name)
    v = _vad(**kw)
    try:
        assert (v.window, v.shift) == (N, shift)
        first, W = len(wav) // 3, 71
        n = N + (W - 1) * shift
        # (b)
        lab, le, thr = v.labels_trials(wav, [(first, n)], return_energy=True)
        singles = [(first + f * shift, N) for f in range(W)]
        _, le1, thr1 = v.labels_trials(wav, singles, return_energy=True)
        assert le.shape == le1.shape == (W,)
        assert np.array_equal(le, le1), np.nonzero(le != le1)[0]
        assert len(np.unique(le)) > W // 2                                               # the frames differ from one another
        # (a)
        for L in vc.invariance_leads(N, shift):
            length = max(n, N + ((L + shift - 1) // shift + 2) * shift + 1)              # the lead ends inside the trial
            led = v.labels_trials(wav, [(first, length)], lead=L, return_energy=True)
            written = np.concatenate([np.zeros(L, np.int16), wav[first:first + length - L]])
            plain = v.labels_trials(written, [(0, length)], return_energy=True)
            assert all(np.array_equal(x, y) for x, y in zip(led, plain)), (name, L)
            assert not np.all(led[1] == led[1][0])                                       # audio behind the zeros
    finally:
        v.close()
