"""The host machinery between a closing speech segment and its audio: dss_amd/segment_queue.py driven directly (through
tests/segment_queue_harness.py: a stub gate, a pass-through decoder, the vocoder's own ragged call as the reference), and
dss_memcpy_d2h_async of csrc/dss_async.cpp against a byte copy.

* healthy schedules at every queue shape: every segment once, a stream's in closing order, PCM equal to the ragged call's, no
  row or event leaked, nothing left open;
* failures injected as Python exceptions while a job is launched, decoded or retired: the failure is sticky, the queue settles,
  close() returns and the library goes on working;
* more segments than pool rows, a collect that raises, close() under a live worker;
* the copy-out kernel's byte tail, its second grid-stride trip, offsets, both kinds of page-locked memory, guard bytes, refusals.

Nothing here provokes a device fault or waits for a time limit: every call that could spin goes through ``within``."""
import ctypes as C_
import functools
import threading

import numpy as np
import pytest
import torch

import segment_queue_harness as H
from dss_amd.lpcnet_weights import synthetic_blob
from segment_queue_harness import CAP, DEADLINE, S, within

pytestmark = pytest.mark.gpu

# (n_lanes, rows_per_job, pool_rows, threaded, progressive)
SHAPES = [(3, 32, None, True, False), (1, 1, 3, True, False), (2, 2, 4, False, False), (1, 1, 3, False, False),
          (2, 2, None, True, True)]


@pytest.fixture(autouse=True, scope="module")
def _model():
    from dss_amd import lpcnet
    lpcnet.load_model(synthetic_blob(0))


def _pool_rows(shape):
    return shape[2] or max(2 * S, 4 * shape[1])


def _lengths(n, pattern):
    return [pattern[k % len(pattern)] for k in range(n)]


def _edges(rows):
    """Two segments of one stream on one tick, a zero-frame segment, one of exactly CAP frames, an empty tick; stream 2 idle."""
    return [[(0, 0, 3), (0, 1, 2)], [(1, 0, 0)], [(1, 1, CAP), (0, 2, 1)], [], [(1, 2, 2)]]


def _full_tick(rows):
    """One tick closes exactly `rows` segments (all three streams in turn), the next tick has to wait for a row."""
    per, tick = [0] * S, []
    for k, n in enumerate(_lengths(rows, (1, 2, 0, 1))):
        tick.append((k % S, per[k % S], n))
        per[k % S] += 1
    return [tick, [(2, per[2], 1)]]


def _backlog(rows):
    """More open segments than rows over consecutive ticks: stream 1 fills the pool, stream 0 closes two more (one of CAP frames)
    on the next tick and stream 1 another on the third; both submits wait for jobs to retire.  Stream 2 idle."""
    return [[(1, k, n) for k, n in enumerate(_lengths(rows, (1, 1, 2, 1)))], [(0, 0, 2), (0, 1, CAP)], [(1, rows, 1)]]


SCHEDULES = {"edges": _edges, "full_tick": _full_tick, "backlog": _backlog}


@functools.lru_cache(maxsize=None)
def _case(name, rows):
    """(schedule, device source, [reference PCM of pass 0, of pass 1]) -- computed once per schedule and pool size, shared by
    every test that uses it, never modified."""
    from dss_amd.lpcnet import LPCNetBatch
    schedule = SCHEDULES[name](rows)
    host = H.make_source(schedule)
    ref = LPCNetBatch(S, CAP)
    want = [H.reference_pcm(schedule, host, ref) for _ in range(2)]
    ref.close()
    return schedule, H.to_device(host), want


def _queue(gate, voc, shape, module=None, **kw):
    from dss_amd.segment_queue import SegmentSynthesisQueue
    n_lanes, per_job, pool, threaded, progressive = shape
    kw.setdefault("decoder_module", module if module is not None else H.PassThrough())
    return SegmentSynthesisQueue(gate, voc, kw.pop("n_features", H.C), CAP, n_lanes=n_lanes, rows_per_job=per_job, pool_rows=pool,
                                 threaded=threaded, progressive=progressive, **kw)


def _close(q, voc):
    try:
        within(DEADLINE, q.close)
    finally:
        voc.close()


# ---- healthy schedules ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCHEDULES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(x) for x in s))
def test_healthy_schedule(shape, name):
    """Two identical passes of a schedule over one queue.  The number of jobs the queue may start while the ticks arrive is
    fixed by the harness (none, except where a submit has to wait for rows), so what a pass needs does not depend on the worker's
    speed: the second pass must get by with the events the first one created."""
    rows = _pool_rows(shape)
    schedule, source, want = _case(name, rows)
    n_seg = len(H.segments_of(schedule))
    assert max(len(t) for t in schedule) <= rows
    gate, voc = H.StubGate(S, source), H.new_vocoder()
    q = _queue(gate, voc, shape)
    try:
        assert q.pool.shape[0] == rows and len(q._free_rows) == rows
        budget = H.LaunchBudget(q)
        n_events = None
        for p in (0, 1):
            segs, chunks = H.run_pass(q, schedule, p, budget)
            H.check_pass(schedule, p, segs, chunks, want[p], shape[4])
            H.assert_settled(q, rows)
            assert q.poll() == []
            if p == 0:
                n_events = len(q._all_events)
                assert 1 <= n_events <= sum(1 for t in schedule if t)
        assert len(q._all_events) == n_events
        assert sorted(q._free_events) == sorted(q._all_events)
        assert len(q.latencies_ms) == 2 * n_seg and q.segments_done == 2 * n_seg
        assert gate.calls == 2 * sum(1 for t in schedule if t)
    finally:
        _close(q, voc)


def test_healthy_schedule_unpaced():
    """The same without the harness's hand on the launches: the worker starts jobs while ticks arrive and poll() runs between
    them (what a host does)."""
    shape = (2, 2, 4, True, True)
    for name in sorted(SCHEDULES):
        schedule, source, want = _case(name, 4)
        voc = H.new_vocoder()
        q = _queue(H.StubGate(S, source), voc, shape)
        try:
            for p in (0, 1):
                segs, chunks = H.run_pass(q, schedule, p)
                H.check_pass(schedule, p, segs, chunks, want[p], True)
                H.assert_settled(q, 4)
            assert len(q._all_events) <= sum(1 for t in schedule if t)
        finally:
            _close(q, voc)


def test_decoder_kernel_lanes():
    """decoder_factory instead of the module: BiLstmDecoderGPU (7 hidden units, 5 inputs) on each lane.  Expected features:
    forward_rows_torch on a handle of its own, bit for bit; they then go through the vocoder reference."""
    import lstm_reference
    from dss_amd.decoder import BiLstmDecoderGPU
    from dss_amd.lpcnet import LPCNetBatch
    sd = lstm_reference.decoder_state_dict(7, 5, 1)
    schedule = _edges(4)
    segs_ = H.segments_of(schedule)
    host = H.make_source(schedule, n_features=5, seed=40)
    pool = torch.zeros((len(segs_), CAP, 5), dtype=torch.float32, device="cuda")
    for i, (s, e, n) in enumerate(segs_):
        if n:
            pool[i, :n] = torch.from_numpy(host[(s, e)]).cuda()
    feats = torch.zeros((len(segs_), CAP, 20), dtype=torch.float32, device="cuda")
    one = BiLstmDecoderGPU(len(segs_), CAP, state_dict=sd)
    one.forward_rows_torch(pool, None, [n for _, _, n in segs_], feats, CAP)
    feats = feats.cpu().numpy()
    ref = LPCNetBatch(S, CAP)
    want = H.reference_pcm(schedule, {(s, e): feats[i, :n] for i, (s, e, n) in enumerate(segs_)}, ref)
    ref.close()
    shape = (2, 2, 4, True, False)
    voc = H.new_vocoder()
    q = _queue(H.StubGate(S, H.to_device(host)), voc, shape, n_features=5, decoder_module=None,
               decoder_factory=lambda r, f: BiLstmDecoderGPU(r, f, state_dict=sd))
    try:
        segs, chunks = H.run_pass(q, schedule, 0)
        H.check_pass(schedule, 0, segs, chunks, want, False)
        H.assert_settled(q, 4)
    finally:
        _close(q, voc)


# ---- failures ---------------------------------------------------------------------------------------------------------------
def _boom(*a, **k):
    raise H.Injected("injected")


def _inject(kind, q, module):
    """-> (n_lanes, rows_per_job) are chosen by the caller; installs the failure."""
    if kind == "launch":                                      # before anything is enqueued
        q._launch = _boom
    elif kind == "decoder":                                   # mid-job: the first row's device work is already on the lane
        module.raise_on = 2
    elif kind == "retire":
        q._retire = _boom
    else:                                                     # the second job fails while the first one's lane is in flight
        real, n = q._launch, [0]

        def second(lane, job):
            n[0] += 1
            if n[0] == 2:
                raise H.Injected("injected")
            return real(lane, job)
        q._launch = second


def _assert_failed_for_good(q, cause, rows):
    """Sticky: three times over, every entry point raises "worker failed" with the original as its cause, and returns."""
    calls = {"submit": lambda: q.submit([2], [0], [1], ["later"]), "empty submit": lambda: q.submit([], [], [], []),
             "poll": q.poll, "poll_chunks": q.poll_chunks, "drain": q.drain}
    for _ in range(3):
        for name, call in calls.items():
            with pytest.raises(RuntimeError, match="worker failed") as ei:
                within(DEADLINE, call)
            assert ei.value.__cause__ is cause, name
    H.assert_settled(q, rows)


@pytest.mark.parametrize("threaded", [True, False], ids=["threaded", "unthreaded"])
@pytest.mark.parametrize("kind", ["launch", "decoder", "retire", "second_job"])
def test_failure_is_sticky_and_the_queue_settles(kind, threaded):
    schedule, source, want = _case("edges", 4)
    source = dict(source)
    source[(2, 0)] = torch.zeros((1, H.C), dtype=torch.float32, device="cuda")
    tick = [(0, 7, CAP), (1, 7, 2)]
    for s, e, n in tick:
        source[(s, e)] = torch.zeros((n, H.C), dtype=torch.float32, device="cuda")
    gate, voc, module = H.StubGate(S, source), H.new_vocoder(), H.PassThrough()
    q = _queue(gate, voc, (2, 1 if kind == "second_job" else 2, 4, threaded, False), module)
    try:
        _inject(kind, q, module)
        within(DEADLINE, lambda: q.submit([t[0] for t in tick], [t[1] for t in tick], [t[2] for t in tick], ["a", "b"]))
        if threaded:                                          # the worker fails; the caller hears of it on its next call
            with pytest.raises(RuntimeError, match="worker failed") as ei:
                within(DEADLINE, q.drain)
            cause = ei.value.__cause__
        else:                                                 # the caller's own thread fails: the exception as it is
            with pytest.raises(H.Injected) as ei:
                within(DEADLINE, q.drain)
            cause = ei.value
        assert isinstance(cause, H.Injected)
        if threaded:
            within(DEADLINE, q._thread.join)                  # the worker is gone, not waiting
        _assert_failed_for_good(q, cause, 4)
        assert gate.calls == 1                                # the refused submits never reached the gate
    finally:
        within(DEADLINE, q.close)
    try:
        assert q.lanes == [] and q._thread is None
        # the library and the vocoder's slots are still good: a new queue on the same vocoder, from fresh slots
        voc.reset()
        torch.cuda.synchronize()
        q2 = _queue(H.StubGate(S, source), voc, (2, 2, 4, threaded, False))
        try:
            segs, chunks = H.run_pass(q2, schedule, 0)
            H.check_pass(schedule, 0, segs, chunks, want[0], False)
            H.assert_settled(q2, 4)
        finally:
            within(DEADLINE, q2.close)
    finally:
        voc.close()


@pytest.mark.parametrize("asynchronous", [True, False], ids=["threaded", "unthreaded"])
def test_pipeline_on_a_failed_queue_raises_every_time(asynchronous):
    """GatedStreamingPipeline.push / flush on top of a failed queue: RuntimeError("worker failed") each time, never a hang."""
    from dss_amd.pipeline import GatedStreamingPipeline
    from test_gpu_gate import _ThresholdVAD
    n_streams, n_ch = 2, 64
    rng = np.random.default_rng(5)
    env = np.concatenate([np.full(200, 20.0), np.full(600, 400.0), np.full(800, 20.0)])
    ecog = rng.standard_normal((n_streams, env.size, n_ch)) * env[None, :, None]
    pipe = GatedStreamingPipeline(n_streams, n_ch, buffer_size=300, context_frames=8, channel_means=np.full(n_ch, 7.4),
                                  vad=_ThresholdVAD(), max_segment_frames=300, asynchronous=asynchronous)
    try:
        pipe.queue._launch = _boom

        def run():
            for k in range(env.size // 40):
                pipe.push(ecog[:, k * 40:(k + 1) * 40])
            pipe.flush()
        with pytest.raises(RuntimeError, match="worker failed" if asynchronous else "injected") as ei:
            within(4 * DEADLINE, run)
        cause = ei.value.__cause__ if asynchronous else ei.value
        assert isinstance(cause, H.Injected)
        for _ in range(3):
            for call in (pipe.flush, pipe.poll, lambda: pipe.push(ecog[:, :40])):
                with pytest.raises(RuntimeError, match="worker failed") as ei:
                    within(DEADLINE, call)
                assert ei.value.__cause__ is cause
        assert pipe.queue.in_flight == 0
    finally:
        within(DEADLINE, pipe.close)
    assert pipe.queue.lanes == [] and pipe.queue._thread is None


# ---- exhaustion and leaks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threaded", [True, False], ids=["threaded", "unthreaded"])
def test_more_segments_than_pool_rows_is_refused_up_front(threaded):
    schedule, source, want = _case("edges", 4)
    source = dict(source)
    for e in range(5):
        source[(2, e)] = torch.zeros((1, H.C), dtype=torch.float32, device="cuda")
    gate, voc = H.StubGate(S, source), H.new_vocoder()
    q = _queue(gate, voc, (2, 2, 4, threaded, False))
    try:
        with pytest.raises(ValueError, match=r"\b5 segments\b.*\b4 rows\b"):
            within(DEADLINE, lambda: q.submit([2] * 5, list(range(5)), [1] * 5, list("abcde")))
        assert gate.calls == 0
        H.assert_settled(q, 4)
        segs, chunks = H.run_pass(q, schedule, 0)             # the next, fitting, submits work
        H.check_pass(schedule, 0, segs, chunks, want[0], False)
        H.assert_settled(q, 4)
    finally:
        _close(q, voc)


@pytest.mark.parametrize("pool_rows", [0, -1])
def test_a_pool_without_rows_is_refused(pool_rows):
    voc = H.new_vocoder()
    try:
        with pytest.raises(ValueError, match="pool_rows"):
            _queue(H.StubGate(S, {}), voc, (1, 1, pool_rows, False, False))
    finally:
        voc.close()


@pytest.mark.parametrize("threaded", [True, False], ids=["threaded", "unthreaded"])
def test_a_collect_that_raises_leaks_neither_rows_nor_event(threaded):
    schedule, source, want = _case("edges", 4)
    gate, voc = H.StubGate(S, source), H.new_vocoder()
    q = _queue(gate, voc, (2, 2, 4, threaded, False))
    try:
        segs, chunks = H.run_pass(q, schedule, 0)
        H.check_pass(schedule, 0, segs, chunks, want[0], False)
        assert q._free_events                                 # so the failing submit has an event to take, and to give back
        before = (list(q._free_rows), list(q._free_events), list(q._all_events), q.in_flight)
        gate.raise_on = gate.calls + 1
        with pytest.raises(H.Injected):
            within(DEADLINE, lambda: q.submit([0, 1], [0, 0], [3, 0], ["x", "y"]))
        assert (list(q._free_rows), list(q._free_events), list(q._all_events), q.in_flight) == before
        H.assert_settled(q, 4)
        segs, chunks = H.run_pass(q, schedule, 1)             # and the queue goes on, bit-exact
        H.check_pass(schedule, 1, segs, chunks, want[1], False)
        H.assert_settled(q, 4)
    finally:
        _close(q, voc)


def test_latency_records_are_bounded():
    voc = H.new_vocoder()
    q = _queue(H.StubGate(S, {}), voc, (1, 1, 3, False, False))
    try:
        for d in (q.latencies_ms, q.first_pcm_latencies_ms, q.lane_wait_ms, q.launch_to_first_pcm_ms):
            assert d.maxlen == 65536
    finally:
        _close(q, voc)


# ---- shutdown under a live worker -------------------------------------------------------------------------------------------
def test_close_refuses_to_free_under_a_live_worker():
    """The worker is held inside _retire (in Python, after its job's event has completed: no GPU work is outstanding).
    close(join_timeout=0.05) must raise and free nothing; once the worker can finish, close() completes and the PCM is there."""
    schedule = [[(0, 0, 2)]]
    host = H.make_source(schedule, seed=70)
    from dss_amd.lpcnet import LPCNetBatch
    ref = LPCNetBatch(S, CAP)
    want = H.reference_pcm(schedule, host, ref)
    ref.close()
    voc = H.new_vocoder()
    q = _queue(H.StubGate(S, H.to_device(host)), voc, (1, 1, 3, True, False))
    entered, release, real = threading.Event(), threading.Event(), q._retire

    def held(lane):
        entered.set()
        if not release.wait(4 * DEADLINE):
            raise H.Injected("the test never released the worker")
        real(lane)
    q._retire = held
    try:
        within(DEADLINE, lambda: q.submit([0], [0], [2], ["tag"]))
        assert entered.wait(DEADLINE), "the job never reached _retire"
        with pytest.raises(RuntimeError, match="still running"):
            within(DEADLINE, lambda: q.close(join_timeout=0.05))
        assert q._thread is not None and q._thread.is_alive()
        assert len(q.lanes) == 1 and q.lanes[0].stream and q.lanes[0].host_ptr and q._all_events
    finally:
        release.set()
    try:
        within(DEADLINE, q.close)
        assert q.lanes == [] and q._thread is None
        out = q.poll()
        assert len(out) == 1 and out[0][:2] == (0, "tag") and np.array_equal(out[0][2], want[(0, 0)])
    finally:
        voc.close()


# ---- dss_memcpy_d2h_async ---------------------------------------------------------------------------------------------------
FULL_GRID = 512 * 256 * 16                                    # bytes one trip of the copy kernel's full grid moves
COPY_SIZES = [0, 1, 15, 16, 17, 31, 4096, 4101, FULL_GRID, FULL_GRID + 16, 2 * FULL_GRID + 57]
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def copy_source():
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    dev = torch.randint(0, 256, (max(COPY_SIZES) + 16,), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    return dev, dev.cpu().numpy()


class _HostBlock:
    def __init__(self, L, nbytes, cached):
        self.L, self.ptr = L, L.dss_host_alloc(nbytes, cached)
        assert self.ptr, L.dss_last_error().decode()
        self.a = np.ctypeslib.as_array((C_.c_uint8 * nbytes).from_address(self.ptr))
        self.a[:] = FILL

    def free(self):
        if self.ptr:
            self.a = None
            self.L.dss_host_free(self.ptr)
            self.ptr = None


def test_copy_sizes_are_the_ones_that_matter():
    assert FULL_GRID == 2_097_152 and COPY_SIZES[-2:] == [2_097_168, 4_194_361]
    assert COPY_SIZES[-1] // 16 > 2 * 512 * 256 - 1 and COPY_SIZES[-1] % 16 == 9        # second trip and a 9-byte tail


@pytest.mark.parametrize("size", COPY_SIZES)
def test_copy_out_against_a_byte_copy(size, copy_source):
    """Every size from the source's base and from base + 16, into cached and coherent page-locked memory at base and base + 16:
    the bytes are the source's, and every byte of the block outside the copy -- the 64 guard bytes behind it and what lies
    before it -- is still 0xA5.  Size 0 leaves the block untouched."""
    from dss_amd import _lib
    L = _lib.require_gpu()
    dev, host = copy_source
    stream = L.dss_stream_create()
    assert stream
    blocks = [_HostBlock(L, 16 + size + GUARD, cached) for cached in (1, 0)]
    try:
        for blk in blocks:
            for src_off in (0, 16):
                for dst_off in (0, 16):
                    blk.a[:] = FILL
                    assert L.dss_memcpy_d2h_async(blk.ptr + dst_off, dev.data_ptr() + src_off, size, stream) == 0, \
                        L.dss_last_error().decode()
                    assert L.dss_stream_synchronize(stream) == 0
                    got = blk.a
                    assert np.array_equal(got[dst_off:dst_off + size], host[src_off:src_off + size]), (src_off, dst_off)
                    assert (got[:dst_off] == FILL).all() and (got[dst_off + size:] == FILL).all(), (src_off, dst_off)
    finally:
        L.dss_stream_synchronize(stream)
        for blk in blocks:
            blk.free()
        L.dss_stream_destroy(stream)


def test_copy_out_refusals(copy_source):
    """A NULL pointer on either side, either pointer off by 8, a pageable destination: an error code, a message, nothing
    written -- and the next good copy is not held to account for it."""
    from dss_amd import _lib
    L = _lib.require_gpu()
    dev, host = copy_source
    n = 4096
    stream = L.dss_stream_create()
    assert stream
    blk = _HostBlock(L, n + GUARD, 1)
    pageable = np.full(n + GUARD + 16, FILL, dtype=np.uint8)
    page_ptr = pageable.ctypes.data + (-pageable.ctypes.data) % 16
    try:
        cases = [("null destination", None, dev.data_ptr(), "null"), ("null source", blk.ptr, None, "null"),
                 ("destination off by 8", blk.ptr + 8, dev.data_ptr(), "aligned"),
                 ("source off by 8", blk.ptr, dev.data_ptr() + 8, "aligned"),
                 ("pageable destination", page_ptr, dev.data_ptr(), "page-locked")]
        for what, dst, src, word in cases:
            rc = L.dss_memcpy_d2h_async(dst, src, n, stream)
            assert rc < 0, what
            msg = L.dss_last_error().decode()
            assert word in msg, (what, msg)
            assert L.dss_stream_synchronize(stream) == 0
            assert (blk.a == FILL).all() and (pageable == FILL).all(), what
            # a good copy after the refusal: the refusal left nothing behind in the runtime
            assert L.dss_memcpy_d2h_async(blk.ptr, dev.data_ptr(), n, stream) == 0, (what, L.dss_last_error().decode())
            assert L.dss_stream_synchronize(stream) == 0
            assert np.array_equal(blk.a[:n], host[:n]) and (blk.a[n:] == FILL).all(), what
            blk.a[:] = FILL
        y = torch.arange(8, device="cuda") + 1                # torch checks the runtime's last error after its own launches
        assert int(y.sum()) == 36
    finally:
        L.dss_stream_synchronize(stream)
        blk.free()
        L.dss_stream_destroy(stream)
