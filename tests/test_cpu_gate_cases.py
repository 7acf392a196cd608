"""The speech-gate case table (tests/gate_cases.py) without a device: oracle/speech_gate_oracle.py replays every stream of every
case of tests/golden/gate_cases.npz (the reference's own VoiceActivityDetectionSmoothing + SpeechSegmentHistory) bit for bit --
its ``threshold`` argument and its windows above 11 labels are held to the reference here for the first time -- and what
every case is there to reach is counted again from the oracle's run and compared with the table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import gate_cases as gc
from speech_gate_oracle import SpeechGateOracle


@pytest.fixture(scope="module")
def fixture(golden):
    g = golden("gate_cases.npz")
    assert tuple(g["names"].tolist()) == gc.NAMES
    return {name: gc.Expected(g, name) for name in gc.NAMES}


@pytest.fixture(scope="module")
def observed():
    return {name: gc.observe(name, SpeechGateOracle) for name in gc.NAMES}


def test_the_table_and_its_generators(fixture):
    assert len(set(gc.NAMES)) == len(gc.NAMES) == 26
    for c in gc.CASES:
        exp = fixture[c.name]
        assert (c.S <= 6 or c.name == "streams_130") and c.pushes <= 400 and 2 * c.smoothing_context + 1 <= 64, c.name
        assert np.array_equal(exp.sizes, gc.sizes(c.name)) and exp.sizes.min() >= 1 and exp.sizes.max() <= c.max_frames, c.name
        for s in range(c.S):
            assert np.array_equal(exp.labels[s], gc.labels(c.name, s)), (c.name, s)
            assert gc.frames(c.name, s).shape == (exp.labels.shape[1], c.C) and gc.frames(c.name, s).dtype == np.float64
    # a stream's data is its own (the written label scripts are shared, the frames never are)
    seeds = {gc.seed(c.name, s) for c in gc.CASES for s in range(-1, c.S) if c.name not in gc.SAME_DATA}
    assert len(seeds) == sum(c.S + 1 for c in gc.CASES if c.name not in gc.SAME_DATA)
    assert not np.array_equal(gc.frames("cap_ctx0_w7", 0), gc.frames("cap_ctx0_w7", 1))
    # the frames are float64 values that the cast has to round; the special values become the bits the table states
    f = gc.frames("mask_33", 0)
    assert not np.array_equal(gc.to_float32(f).astype(np.float64), f)
    want = np.array([b for _, b in gc.SPECIAL], dtype=np.uint32)
    assert np.array_equal(gc.bits(gc.to_float32(np.array([v for v, _ in gc.SPECIAL]))), want)
    assert np.float64(gc.SPECIAL[7][0]) > gc.HALF_SUBNORMAL == 2.0 ** -150 and np.isnan(gc.SPECIAL[-1][0])
    assert np.array([gc.SPECIAL[-1][0]]).view(np.uint64)[0] == 0x7ff8000000000000
    # the capacity formula, restated: the scripts of the capacity cases are what it allows at most
    assert [gc.max_events(w, ctx) for w, ctx in ((7, 0), (8, 0), (8, 2), (1, 0), (1, 2), (50, 2), (6, 2))] == [4, 4, 3, 1, 1, 17, 3]
    # the window of the refusal is the first one a 64-bit mask cannot hold
    assert 2 * gc.REFUSED_SMOOTHING_CONTEXT + 1 == 65 and 2 * gc.case("mask_63").smoothing_context + 1 == 63


@pytest.mark.parametrize("name", gc.NAMES)
def test_oracle_replays_the_reference(fixture, name):
    c = gc.case(name)
    oracles = [SpeechGateOracle(c.C, c.N, c.context, c.smoothing_context, c.threshold) for _ in range(c.S)]

    def push(frames, labels):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            got = [o.push(frames[s], labels[s]) for s, o in enumerate(oracles)]
        return [g[0] for g in got], [g[1] for g in got]
    gc.replay(fixture[name], push)
    assert all(o.frames_seen == int(gc.sizes(name).sum()) for o in oracles)


@pytest.mark.parametrize("name", gc.NAMES)
def test_every_case_reaches_what_it_is_there_for(fixture, observed, name):
    c = gc.case(name)
    o, _ = observed[name]
    assert {k: o[k] for k, _ in c.reach} == dict(c.reach), name
    assert o["segments"] == fixture[name].n_segments
    assert o["most_in_a_push"] <= gc.max_events(c.max_frames, c.context)


def test_reach_by_kind(observed):
    """What the issue of each group of cases is, stated on the table itself: were a reach column edited to agree with a case that
    no longer reaches its branch, this fails."""
    r = {c.name: dict(c.reach) for c in gc.CASES}
    assert r["mask_33"]["bit_32"] is True and r["mask_63"]["bit_62"] is True
    assert r["thr_one_49"]["count_49_of_49"] is True and r["thr_one_49"]["count_48_of_49"] is True
    assert 49 * (1.0 / 49.0) < 1.0 <= 49 / 49.0                   # what the division is there for
    assert r["thr_zero"] == {"segments": 0, "all_speech": True} and r["thr_above_one"] == {"segments": 0, "no_speech": True}
    for name, count in gc.TIE_COUNT.items():
        c = gc.case(name)
        assert count / (2 * c.smoothing_context + 1) >= c.threshold > (count - 1) / (2 * c.smoothing_context + 1)
        assert count / (2 * c.smoothing_context + 1) == c.threshold and r[name]["on_tie"] > 0 and r[name]["segments"] > 40, name
    assert r["zero_ctx1"]["empty_segments"] >= 1 and r["zero_ctx0"]["empty_segments"] >= 2
    for name in ("cap_ctx0_w7", "cap_ctx0_w8", "cap_ctx2_w8"):
        c = gc.case(name)
        assert r[name]["most_in_a_push"] == gc.max_events(c.max_frames, c.context), name
    # the widths: dr = 256 / C and dc = 256 mod C take every combination of zero and non-zero; totals under one step, inside the
    # unroll (not a multiple of 256) and over several trips of the 1024-element step
    assert sorted(gc.case(n).C for n in gc.WIDTH_NAMES) == [1, 63, 64, 65, 255, 256, 257, 300]
    steps = {(gc.THREADS // gc.case(n).C > 0, gc.THREADS % gc.case(n).C > 0) for n in gc.WIDTH_NAMES}
    assert steps == {(True, False), (True, True), (False, True)}
    for n in gc.WIDTH_NAMES:
        el = observed[n][0]["element_counts"]
        assert 14 <= len(el) and gc.case(n).N == 41 and max(el) // gc.case(n).C <= 40, n
        assert r[n]["above_1024"] is (gc.case(n).C > 1) and r[n]["not_multiple_of_256"] is (gc.case(n).C != 256), n
    assert min(min(observed[n][0]["element_counts"]) for n in gc.WIDTH_NAMES) < gc.THREADS
    assert max(observed["width_300"][0]["element_counts"]) > 3 * gc.UNROLL * gc.THREADS
    tails = {(e % (gc.UNROLL * gc.THREADS)) // gc.THREADS for n in gc.WIDTH_NAMES for e in observed[n][0]["element_counts"]}
    assert tails == {0, 1, 2, 3}                                   # totals that end in every step of the 4-wide unroll
    assert r["values"]["special_values_emitted"] == len(gc.SPECIAL) == 14
    assert r["long_64"]["above_4096"] is True and gc.case("long_64").C == 64
    assert r["streams_130"]["streams_closing_on_last_run"] == gc.case("streams_130").S == 130


def test_one_by_one_and_whole_push_give_the_same_segments(fixture, observed):
    a, b = fixture["one_by_one"], fixture["whole_50"]
    assert gc.case("one_by_one").max_frames == 1 and gc.case("whole_50").pushes == 1 and a.n_segments == b.n_segments > 0
    for s in range(2):
        assert np.array_equal(gc.frames("one_by_one", s), gc.frames("whole_50", s))
        assert np.array_equal(gc.labels("one_by_one", s), gc.labels("whole_50", s))
        rows_a = [x for k in range(50) for x in a.rows_of(s, k)]
        rows_b = b.rows_of(s, 0)
        assert len(rows_a) == len(rows_b) and all(np.array_equal(x, y) for x, y in zip(rows_a, rows_b))
        assert int(a.speech[s].sum()) == int(b.speech[s, 0])
        got_a = [x for segs, _ in observed["one_by_one"][1][s] for x in segs]
        got_b = [x for segs, _ in observed["whole_50"][1][s] for x in segs]
        assert len(got_a) == len(got_b) == len(rows_b) and all(np.array_equal(x, y) for x, y in zip(got_a, got_b))
