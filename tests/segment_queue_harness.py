"""A direct harness for dss_amd.segment_queue.SegmentSynthesisQueue: the queue without the pipeline around it.

Through GatedStreamingPipeline a test cannot choose which segments close on which tick.  The queue itself only needs ``gate.S`` and
``gate.collect_torch(streams, events, rows, pool, hip_stream=...)``, so a stub gate that copies prepared segments into the pool, a
decoder module that hands its input through, and the vocoder's own ragged call as the reference are enough to drive it with any
schedule.  A schedule is a list of ticks, a tick a list of (stream, event, length); ``event`` numbers a stream's segments in
closing order over the whole schedule, so (stream, event) names one segment.

Every call of the queue that can wait (submit, drain, flush, close) goes through ``within``: a queue that spins shows as a failed
assertion, never as a stuck test."""
import threading

import numpy as np
import pytest
import torch

from dss_amd.lpcnet import FRAME_SIZE, LPCNetBatch
from dss_amd.lpcnet_weights import synthetic_features

S, C, CAP = 3, 20, 4
# A cap, not a measurement: the largest schedule here is well under 0.1 s of device work (0.39 ms per vocoder frame), so any
# finite bound separates "returns" from "spins".
DEADLINE = 5.0


def within(seconds, fn):
    """fn() on a daemon thread, joined with a deadline: fails the test with "did not return" when the thread is still alive,
    otherwise returns fn's result or re-raises its exception."""
    box = {}

    def run():
        try:
            box["result"] = fn()
        except BaseException as e:                            # handed to the caller's thread below
            box["error"] = e
    th = threading.Thread(target=run, name="within", daemon=True)
    th.start()
    th.join(seconds)
    if th.is_alive():
        pytest.fail(f"{getattr(fn, '__qualname__', fn)} did not return within {seconds} s")
    if "error" in box:
        raise box["error"]
    return box.get("result")


class Injected(RuntimeError):
    """What the stubs and the tests raise on purpose."""


class StubGate:
    """The two things the queue takes from a SpeechGateGPU.  ``source[(stream, event)]`` is that segment's (length, C) float32 CUDA
    tensor; collect_torch copies it into pool[row, :length] on the stream it is given.  ``raise_on = k`` makes the k-th call
    raise before it copies anything; ``calls`` counts them."""

    def __init__(self, n_streams, source):
        self.S, self.source = int(n_streams), source
        self.calls, self.raise_on = 0, None

    def collect_torch(self, streams, events, dst_rows, pool, hip_stream=None):
        self.calls += 1
        if self.calls == self.raise_on:
            raise Injected(f"collect call {self.calls}")
        cur = torch.cuda.current_stream()
        on = cur if hip_stream is None or hip_stream == cur.cuda_stream else torch.cuda.ExternalStream(hip_stream)
        with torch.cuda.stream(on), torch.no_grad():
            for s, e, r in zip(streams, events, dst_rows):
                x = self.source[(int(s), int(e))]
                if x.shape[0]:
                    pool[int(r), : x.shape[0]].copy_(x)


class PassThrough(torch.nn.Module):
    """A decoder module with the reference's call signature that returns its input: with n_features = n_out = 20 the vocoder sees
    exactly the stub gate's rows.  ``raise_on = k`` makes the k-th call raise."""

    def __init__(self):
        super().__init__()
        self.calls, self.raise_on = 0, None

    def create_new_initial_state(self, batch_size, device="cpu"):
        return None

    def forward(self, x, state=None):
        self.calls += 1
        if self.calls == self.raise_on:
            raise Injected(f"decoder call {self.calls}")
        return x, state


class LaunchBudget:
    """Lets a test say how many jobs the queue may start, so that what a pass needs (events, rows) does not depend on how fast
    the worker thread happens to be.  It stands in front of ``_take_job`` (called with the queue's lock held): with nothing
    allowed no job is taken, and nothing blocks.  ``allow(None)`` lifts the limit."""

    def __init__(self, queue, allowed=0):
        self.q, self.allowed, self._take = queue, allowed, queue._take_job
        queue._take_job = self._take_job

    def _take_job(self):
        if self.allowed == 0:
            return []
        job = self._take()
        if job and self.allowed is not None:
            self.allowed -= 1
        return job

    def allow(self, n):
        with self.q._cv:
            self.allowed = None if n is None or self.allowed is None else self.allowed + n
            self.q._cv.notify_all()

    def hold(self):
        with self.q._cv:
            self.allowed = 0

    def remove(self):
        self.q._take_job = self._take


def segments_of(schedule):
    return [seg for tick in schedule for seg in tick]


def make_source(schedule, n_features=C, seed=0):
    """{(stream, event): (length, n_features) float32 host array}: LPCNet features (``synthetic_features``) for 20 columns, normal
    deviates otherwise (the input of a decoder)."""
    out = {}
    for s, e, n in segments_of(schedule):
        assert (s, e) not in out, "a stream's events are numbered once over the schedule"
        if n_features == 20:
            out[(s, e)] = synthetic_features(seed + 100 * s + e, n)
        else:
            out[(s, e)] = np.random.default_rng(seed + 100 * s + e).standard_normal((n, n_features)).astype(np.float32)
    return out


def to_device(source):
    dev = {k: torch.from_numpy(v).cuda() for k, v in source.items()}
    torch.cuda.synchronize()
    return dev


def reference_pcm(schedule, features, batch):
    """{(stream, event): int16 PCM} of one pass over `schedule` on `batch` (an LPCNetBatch(S, CAP) of its own, whose slots carry
    over to the next pass): every stream's segments one ``synthesize_ragged(..., slots=[stream])`` call at a time, in closing
    order.  That path is held to the oracle bit for bit by test_gpu_lpcnet.py::test_ragged_rows_and_slot_indexed_state.
    features[(stream, event)]: (length, 20) float32 host array."""
    out = {}
    for s, e, n in segments_of(schedule):
        f = np.asarray(features[(s, e)], dtype=np.float32)
        assert f.shape == (n, 20)
        out[(s, e)] = batch.synthesize_ragged([f], slots=[s])[0]
        assert out[(s, e)].shape == (n * FRAME_SIZE,)
    return out


def run_pass(queue, schedule, pass_id=0, budget=None):
    """One pass over `schedule`: a submit per tick (tags (pass_id, stream, event)), then drain.  With a LaunchBudget the queue
    starts no job while the ticks arrive, except the ones a submit has to wait for (a tick that needs more rows than are free),
    and the limit is lifted before the drain.  Returns (segments as poll()/drain() handed them out, pieces of poll_chunks())."""
    segs, chunks = [], []
    if budget is not None:
        budget.hold()
    for tick in schedule:
        streams, events, lengths = [t[0] for t in tick], [t[1] for t in tick], [t[2] for t in tick]
        tags = [(pass_id, s, e) for s, e, _ in tick]
        if budget is not None:
            with queue._cv:
                short = len(tick) - len(queue._free_rows)
            if short > 0:                                     # every job gives back at least one row
                budget.allow(short)
        within(DEADLINE, lambda: queue.submit(streams, events, lengths, tags))
        if budget is not None:
            budget.hold()
        else:
            segs += queue.poll()
            if queue.progressive:
                chunks += queue.poll_chunks()
    if budget is not None:
        budget.allow(None)
    segs += within(DEADLINE, queue.drain)
    if queue.progressive:
        chunks += queue.poll_chunks()
    return segs, chunks


def check_pass(schedule, pass_id, segs, chunks, want, progressive):
    """Every segment of the pass exactly once with its tag, a stream's in closing order, PCM equal to `want`; progressive: the
    pieces of each segment run contiguously from 0, concatenate to it, and exactly one -- the final one -- is ``last``."""
    expect = [(pass_id, s, e) for s, e, _ in segments_of(schedule)]
    assert sorted(tag for _, tag, _ in segs) == sorted(expect)
    order = {}
    for s, tag, pcm in segs:
        assert tag[1] == s and pcm.dtype == np.int16
        order.setdefault(s, []).append(tag[2])
        assert np.array_equal(pcm, want[(tag[1], tag[2])]), tag
    for s, evs in order.items():
        assert evs == sorted(evs), (s, evs)
    if not progressive:
        assert chunks == []
        return
    pieces, lasts, seq = {}, {}, {}
    for s, tag, off, pcm, last in chunks:
        assert tag[1] == s and pcm.dtype == np.int16
        assert lasts.get(tag, 0) == 0, ("a piece after the last one", tag)
        got = pieces.setdefault(tag, [])
        assert off == sum(len(x) for x in got), (tag, off)
        got.append(pcm)
        lasts[tag] = lasts.get(tag, 0) + bool(last)
        if not seq.setdefault(s, []) or seq[s][-1] != tag[2]:
            seq[s].append(tag[2])
    assert sorted(pieces) == sorted(expect)
    for tag in expect:
        assert lasts[tag] == 1, tag
        assert np.array_equal(np.concatenate(pieces[tag]), want[(tag[1], tag[2])]), tag
    for s, evs in seq.items():
        assert evs == sorted(set(evs)), (s, evs)              # all of a segment before any of the stream's next one


def assert_settled(queue, rows):
    """Nothing open, nothing busy, every pool row free exactly once, no lane holds a job."""
    assert queue.in_flight == 0
    assert not queue.busy.any()
    assert sorted(queue._free_rows) == list(range(rows))
    assert all(lane.job is None for lane in queue.lanes)
    assert not queue.pending


def new_vocoder():
    return LPCNetBatch(S, 1)
