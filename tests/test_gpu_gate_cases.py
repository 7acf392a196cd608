"""GPU tests of the speech-gate kernels (csrc/speech_gate.hip, csrc/dss_gate.cpp) over the case table of tests/gate_cases.py:
``SpeechGateGPU.push`` / ``push_torch`` + ``segment_torch`` against tests/golden/gate_cases.npz (the reference's own classes) bit
for bit, ``collect_torch`` directly against the same rows, and ``reset`` against a fresh oracle (oracle/speech_gate_oracle.py,
which tests/test_cpu_gate_cases.py holds to the same fixture)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import numpy as np
import pytest
import torch

import gate_cases as gc

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def fixture(golden):
    g = golden("gate_cases.npz")
    assert tuple(g["names"].tolist()) == gc.NAMES
    return {name: gc.Expected(g, name) for name in gc.NAMES}


def _gate(c, S=None):
    from dss_amd.gate import SpeechGateGPU
    return SpeechGateGPU(S or c.S, c.C, c.N, c.context, c.smoothing_context, c.threshold, max_frames=c.max_frames)


def _dev(frames, labels):
    return torch.from_numpy(np.ascontiguousarray(frames)).cuda(), torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()


@pytest.mark.parametrize("name", gc.NAMES)
def test_push_over_the_table(fixture, name):
    """Every case, all streams at once, through the host-buffer entry and once more through the device-resident one: per push the
    same number of segments, lengths, speech counts and rows as the reference's classes gave, bit for bit (uint32 views)."""
    c, exp = gc.case(name), fixture[name]
    total = int(gc.sizes(name).sum())
    gate = _gate(c)
    assert gate.E == gc.max_events(c.max_frames, c.context)
    gc.replay(exp, gate.push)
    assert [gate.frames_seen(s) for s in (0, c.S - 1)] == [total, total]
    gate.close()

    gate = _gate(c)

    def push_dev(frames, labels):
        ev = gate.push_torch(*_dev(frames, labels))
        segs = [[gate.segment_torch(s, e).cpu().numpy() for e in range(int(ev[s, 0]))] for s in range(c.S)]
        assert all(len(seg) == int(ev[s, 2 + e]) for s in range(c.S) for e, seg in enumerate(segs[s]))
        return segs, ev[:, 1].copy()
    gc.replay(exp, push_dev)
    assert [gate.frames_seen(s) for s in (0, c.S - 1)] == [total, total]
    gate.close()


def test_the_first_window_the_mask_cannot_hold_is_refused():
    from dss_amd import _lib
    from dss_amd.gate import SpeechGateGPU
    c = gc.case("mask_63")
    with pytest.raises(_lib.DssError, match="<= 64"):
        SpeechGateGPU(c.S, c.C, c.N, c.context, gc.REFUSED_SMOOTHING_CONTEXT, c.threshold, max_frames=c.max_frames)


# ---- collect_torch -----------------------------------------------------------------------------------------------------------
def _run_to_push(name, last, S=None):
    """A gate of the case (with S streams: the written label scripts are shared by any number of streams, each with frames of
    its own) pushed through push_torch up to and including push ``last`` -> (gate, host event table of that push)."""
    c = gc.case(name)
    gate = _gate(c, S)
    for k in range(last + 1):
        f, lab = gc.push_inputs(name, k, range(S or c.S))
        ev = gate.push_torch(*_dev(f, lab))
    return gate, ev.copy()


def _wanted(exp, name, last, S):
    """[(stream, event, float32 rows)] of every segment push ``last`` closes.  Streams beyond the fixture's own run the same
    label script, so their segments copy the same frame indices -- of their own frames."""
    c = exp.case
    out = []
    for s in range(S):
        for e, index in enumerate(exp.rows_of(s if s < c.S else 0, last)):
            out.append((s, e, gc.rows_from(gc.frames32(name, s), index)))
    return out


def _pool(rows, row_frames, C):
    return torch.full((rows, row_frames, C), float(SENTINEL), dtype=torch.float32, device="cuda")


def _check_pool(pool, picked, dst_rows):
    """Named rows hold their segment and then the sentinel, every other row the sentinel alone."""
    got = gc.bits(pool.cpu().numpy())
    sent = gc.bits(np.array([SENTINEL]))[0]
    untouched = np.ones(got.shape[0], dtype=bool)
    for (s, e, seg), r in zip(picked, dst_rows):
        assert np.array_equal(got[r, :len(seg)], gc.bits(seg)), (s, e, r)
        assert np.all(got[r, len(seg):] == sent), (s, e, r, "the tail of the row was written")
        untouched[r] = False
    assert np.all(got[untouched] == sent)


def _collect_and_check(gate, wanted, n, extra_frames, seed):
    rng = np.random.default_rng(seed)
    picked = [wanted[i] for i in sorted(rng.permutation(len(wanted))[:n].tolist())]
    C = gate.C
    longest = max([len(seg) for _, _, seg in picked] + [1])
    rows = 2 * n + 3
    dst = rng.permutation(rows)[:n]                                  # a permutation with gaps
    pool = _pool(rows, longest + extra_frames, C)
    gate.collect_torch([s for s, _, _ in picked], [e for _, e, _ in picked], dst, pool)
    torch.cuda.synchronize()
    _check_pool(pool, picked, dst.tolist())
    return picked, dst, pool


@pytest.mark.parametrize("n", [0, 1, 64, 65, 130])
def test_collect_130_streams_closing_on_one_push(fixture, n):
    """0, 1, DSS_GATE_COLLECT_MAX, one more (a second launch of one segment) and all 130 segments of the push on which every stream
    of ``streams_130`` closes one; destination rows exactly as long as the longest segment and three frames longer."""
    name = "streams_130"
    exp, c = fixture[name], gc.case(name)
    last = max(k for (_, k) in exp.segments)
    wanted = _wanted(exp, name, last, c.S)
    assert len(wanted) == c.S == 130 and len({len(seg) for _, _, seg in wanted}) > 3
    gate, ev = _run_to_push(name, last)
    assert np.all(ev[:, 0] == 1)
    for extra in (0, 3):
        _collect_and_check(gate, wanted, n, extra, 100 * n + extra)
    gate.close()


@pytest.mark.parametrize("n", [1, 64, 65, 132])
def test_collect_several_events_per_stream(fixture, n):
    """33 streams of ``cap_ctx0_w7``: the push that closes max_events = 4 segments in every stream, 132 in all (three launches)."""
    name, S = "cap_ctx0_w7", 33
    exp = fixture[name]
    assert np.array_equal(exp.labels[0], exp.labels[1])
    last = 1
    wanted = _wanted(exp, name, last, S)
    assert len(wanted) == 4 * S and {e for _, e, _ in wanted} == {0, 1, 2, 3}
    gate, ev = _run_to_push(name, last, S)
    assert gate.E == 4 and np.all(ev[:, 0] == 4)
    for extra in (0, 2):
        _collect_and_check(gate, wanted, n, extra, 7 * n + extra)
    gate.close()


def test_collect_long_empty_repeated_and_on_a_side_stream(fixture):
    # a segment of 104 x 64 = 6656 elements: the second trip of the kernel's stride loop (16 x 256 elements a trip)
    name = "long_64"
    exp = fixture[name]
    last = max(k for (_, k) in exp.segments)
    wanted = _wanted(exp, name, last, 2)
    assert [seg.size for _, _, seg in wanted] == [6656, 6656] and 6656 > gc.COLLECT_ROWS * gc.THREADS
    gate, _ = _run_to_push(name, last)
    picked, dst, pool = _collect_and_check(gate, wanted, 2, 5, 1)
    # the same push collected again gives the same rows
    again = _pool(*pool.shape)
    gate.collect_torch([s for s, _, _ in picked], [e for _, e, _ in picked], dst, again)
    torch.cuda.synchronize()
    assert torch.equal(pool.view(torch.int32), again.view(torch.int32))
    gate.close()

    # push and collect issued under a side stream
    side = torch.cuda.Stream()
    gate = _gate(gc.case(name))
    inputs = [_dev(*gc.push_inputs(name, k)) for k in range(last + 1)]
    on_side = _pool(*pool.shape)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for f, lab in inputs:
            ev = gate.push_torch(f, lab)
        assert ev[:, 0].tolist() == [1, 1]
        gate.collect_torch([s for s, _, _ in picked], [e for _, e, _ in picked], dst, on_side)
    side.synchronize()
    _check_pool(on_side, picked, dst.tolist())
    gate.close()

    # segments of 0 rows: nothing is written, whatever the row
    for name in ("zero_ctx1", "zero_ctx0"):
        exp = fixture[name]
        empties = sorted(k for (s, k), segs in exp.segments.items() if s == 0 and any(len(x) == 0 for x in segs))
        assert empties
        for last in empties:
            wanted = _wanted(exp, name, last, 2)
            assert [len(seg) for _, _, seg in wanted] == [0, 0]
            gate, ev = _run_to_push(name, last)
            assert ev[:, 0].tolist() == [1, 1] and ev[:, 2].tolist() == [0, 0]
            _collect_and_check(gate, wanted, 2, 0, last)
            gate.close()


def test_collect_refusals(fixture):
    from dss_amd import _lib
    name = "streams_130"
    exp, c = fixture[name], gc.case(name)
    last = max(k for (_, k) in exp.segments)
    wanted = _wanted(exp, name, last, c.S)
    gate, ev = _run_to_push(name, last)
    length = len(wanted[5][2])
    pool = _pool(4, max(len(seg) for _, _, seg in wanted), c.C)
    with pytest.raises(_lib.DssError, match="asked for #1"):
        gate.collect_torch([5], [1], [0], pool)                      # an event index at the count
    with pytest.raises(_lib.DssError, match="asked for #7"):
        gate.collect_torch([4, 5], [0, 7], [0, 1], pool)             # ... and beyond it, behind a good one
    with pytest.raises(_lib.DssError, match="buffer holds %d" % (length - 1)):
        gate.collect_torch([5], [0], [0], _pool(4, length - 1, c.C))
    with pytest.raises(_lib.DssError, match="negative destination row"):
        gate.collect_torch([5], [0], [-1], pool)
    for bad in (c.S, -1):
        with pytest.raises(_lib.DssError, match="bad gate/stream/event"):
            gate.collect_torch([bad], [0], [0], pool)
    with pytest.raises(_lib.DssError, match="bad gate/stream/event"):
        gate.collect_torch([5], [-1], [0], pool)
    with pytest.raises(ValueError, match="rows inside the pool"):
        gate.collect_torch([5], [0], [4], pool)
    with pytest.raises(ValueError, match="one entry per segment"):
        gate.collect_torch([5, 6], [0], [0, 1], pool)
    torch.cuda.synchronize()
    _check_pool(pool, [], [])                                        # no refused call wrote anything
    gate.collect_torch([5], [0], [2], pool)                          # and the gate still collects
    torch.cuda.synchronize()
    _check_pool(pool, [wanted[5]], [2])
    gate.close()


# ---- reset ------------------------------------------------------------------------------------------------------------------
def test_reset_returns_a_stream_to_a_fresh_gate():
    """A full window of speech labels and a run in progress, then reset(1): stream 1 returns on the following pushes exactly what
    a fresh oracle returns -- with the zero rows of the emptied rings in its first segment -- while streams 0 and 2 go on; then
    reset() does it for all three."""
    from dss_amd.gate import SpeechGateGPU
    from speech_gate_oracle import SpeechGateOracle
    S, C, N, ctx, sm, W = 3, 5, 16, 2, 2, 6
    rng = np.random.default_rng(4242)
    gate = SpeechGateGPU(S, C, N, ctx, sm, 0.6, max_frames=W)
    fresh = lambda: SpeechGateOracle(C, N, ctx, sm, 0.6)
    host = [fresh() for _ in range(S)]
    n_seg, zero_rows = [0] * S, [0] * S

    def push(labels):
        nonlocal zero_rows
        f = rng.standard_normal((S, len(labels), C)) * 3.0
        lab = np.tile(np.asarray(labels), (S, 1))
        got, n_speech = gate.push(f, lab)
        for s in range(S):
            want, want_speech = host[s].push(f[s], lab[s])
            assert len(got[s]) == len(want) and int(n_speech[s]) == want_speech, s
            for a, b in zip(got[s], want):
                assert a.shape == b.shape and np.array_equal(gc.bits(a), gc.bits(b)), s
                zero_rows[s] += int(np.sum(~a.any(axis=1)))
            n_seg[s] += len(want)
            assert gate.frames_seen(s) == host[s].frames_seen

    script = ([1, 1, 1, 0, 0, 0], [0, 0, 0], [1, 1, 1, 1, 1, 1], [1, 0, 0, 0, 0, 0], [0, 0, 1, 1, 1, 0], [0, 0, 0, 0, 0, 0])
    push([1, 1, 1, 0, 0, 0])
    push([0] * 6)                                                    # every stream has closed the segment that holds its first, zero rows
    assert min(n_seg) == 1 and min(zero_rows) > 0
    push([1] * 6)
    push([1] * 5)
    assert all(sum(h.win_labels) == 5 and h.speech > 0 for h in host)          # the window is full, a run is in progress
    gate.reset(1)
    host[1] = fresh()
    zero_rows = [0] * S
    assert gate.frames_seen(1) == 0 and gate.frames_seen(0) == 23
    for labels in script:
        push(labels)
    assert min(n_seg) >= 3 and zero_rows[1] > 0 and zero_rows[0] == zero_rows[2] == 0
    push([1] * 6)
    gate.reset()
    host = [fresh() for _ in range(S)]
    before = list(zero_rows)
    for labels in script:
        push(labels)
    assert all(z > b for z, b in zip(zero_rows, before))
    gate.close()
