"""The HGA case table (tests/hga_cases.py) without a device: the plan of every case as the library reports it (``dss_hga_plan``,
the helper dss_launch_hga and dss_launch_hga_trials size their launches by), the plan's invariants over a sweep of window
shapes, and the references the GPU tests lean on, each pinned to something independent of this repository's kernels -- the
oracle's cascades to scipy at every filter order of the table, the oracle's frame counts to the table, the host twins of the
patch and statistics kernels to numpy at the new neighbour counts and sizes, the front-end reference to the reference's own
classes (tests/golden/ecog_chain.npz).  Everything is array_equal; nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import hga_cases as hc
from dss_amd import _lib, electrodes, hga, session


def test_plan_of_every_case_equals_the_table():
    for c in hc._TABLE:
        p = hga.plan(c.fs, c.wl, c.ws)
        assert tuple(p) == c.plan, (c.name, tuple(p))
        assert p.ring_rows == hc.ring_rows(p.frame_length, p.shift) and p.ring_bytes == 128 * p.ring_rows
        assert p.overlap == p.frame_length - p.shift
    # the cases sit where they claim to: the reference's shape, the two sides of the ring's edge, a table that is too short
    assert tuple(hga.plan()) == hc._D == (50, 10, 40, 128, 16384, 1)
    last, first = hc.case("ring_last_fused_8").plan, hc.case("ring_first_fallback_8").plan
    assert last[3:] == (320, hc.RING_LIMIT, 1) and first[3:] == (328, hc.RING_LIMIT + 1024, 0) and first[1] == last[1] + 1
    assert {hc.case(n).plan[5] for n in hc.names("orders") + hc.names("tails") + hc.names("table")} == {1}
    assert max(hc.case("beyond_table").frames) > hc.WTAB
    for c in hc._TABLE:                       # the first packet is shorter than a frame, and for the orders than the pipeline
        assert c.packets[0] < c.plan[0] or c.group == "table"
    # 3 rows: fewer than the 2 nsec - 1 steps the pipeline needs to fill from order 3 on, exactly as many at order 2
    assert all(hc.case(n).packets[0] < 2 * hc.case(n).order - 1 for n in hc.names("orders") if hc.case(n).order >= 3)
    assert all(min(hc.case(n).packets) < hc.case(n).plan[2] for n in hc.names("tails"))
    # blocks of 16 columns that hold two or three streams; a partial channel group of the window kernel behind a full one
    for n in hc.names("tails"):
        c = hc.case(n)
        streams = [len({p // c.C for p in range(b, min(b + 16, c.S * c.C))}) for b in range(0, c.S * c.C, 16)]
        assert max(streams) >= 2 and c.C % 16
    assert 32 < hc.case("tail_3x40").C < 64 and (7 * 5) % 16 == 3


def test_plan_invariants_over_a_sweep():
    L = _lib.load()
    seen = set()
    for fs in (250, 512, 1000, 2000, 8000):
        for wl in (0.025, 0.05, 0.1, 0.375, 0.3):
            fused = []
            for ws in np.linspace(0.005, wl, 23):
                p = hga.plan(fs, wl, float(ws))
                assert p.fused == int(p.ring_bytes <= hc.RING_LIMIT) and p.ring_bytes == 128 * p.ring_rows
                assert p.ring_rows % 8 == 0 and p.frame_length + p.shift + 66 <= p.ring_rows < p.frame_length + p.shift + 66 + 8
                assert 0 < p.shift <= p.frame_length and p.overlap == p.frame_length - p.shift
                # the float32 products of the reference's frame buffer
                assert p.frame_length == int(np.float32(wl) * np.float32(fs)) and p.shift == int(np.float32(ws) * np.float32(fs))
                fused.append(p.fused)
                seen.add(p.fused)
            assert fused == sorted(fused, reverse=True), (fs, wl)          # a longer shift never brings the one-launch form back
    assert seen == {0, 1}
    # along the shift at the ring-edge shape the form flips exactly once, between the two cases of the table
    flips = []
    for shift in range(1, 193):
        p = hga.plan(512, 0.375, shift / 512)
        assert p.frame_length == 192 and p.shift == shift
        flips.append(p.fused)
    assert flips == [1] * 62 + [0] * 130
    # refusals: no shift, a shift beyond the frame, no frame, no sampling rate, nowhere to write
    out = (C.c_int * 6)()
    for fs, wl, ws in ((1000, 0.05, 0.0), (1000, 0.05, 0.051), (1000, 0.0, 0.0), (0, 0.05, 0.01), (1000, 0.05, -0.01)):
        assert L.dss_hga_plan(fs, wl, ws, C.addressof(out)) < 0 and b"window shape" in L.dss_last_error(), (fs, wl, ws)
        with pytest.raises(_lib.DssError):
            hga.plan(fs, wl, ws)
    assert L.dss_hga_plan(1000, 0.05, 0.01, None) < 0 and b"nowhere to write the plan" in L.dss_last_error()


def test_tile_bounds_follow_the_codes_formulas():
    """The largest front end and wire packet of the table, from the launch code's own byte counts
    (dss_launch_hga_frontend: (32 c_raw + 128) doubles + 4 c_raw ints; dss_launch_hga_wire: C n floats; both <= 64 KB)."""
    def front_bytes(c_raw):
        return (32 * c_raw + 32 * 4) * 8 + 4 * c_raw * 4
    assert front_bytes(hc.FRONT_MAX_C_RAW) <= 65536 < front_bytes(hc.FRONT_MAX_C_RAW + 1) and hc.FRONT_MAX_C_RAW == 237
    assert hc.front("front_largest").c_raw == hc.FRONT_MAX_C_RAW
    for c, n, ok in hc.WIRE:
        assert hc.wire_fits(c, n) == ok, (c, n)
    assert 129 * 127 * 4 == 65532 and hc.wire_fits(129, 127) and not hc.wire_fits(129, 128)
    assert 64 * 256 * 4 == hc.WIRE_LIMIT and not hc.wire_fits(64, 257)
    sizes = sorted(len(m) for f in hc.FRONTS for m in f.comp_lists)
    assert {1, 7, 8, 9, 17} <= set(sizes)
    assert sorted(len(f.comp_lists) for f in hc.FRONTS) == [1, 2, 2, 2, 3, 4]
    f = hc.front("front_unreferenced")
    assert (f.grid_of == -1).sum() * 3 == f.C
    f = hc.front("front_repeated_source")
    assert len(set(f.src_col.tolist())) == f.C - 1
    for f in hc.FRONTS:
        assert f.src_col.max() < f.c_raw and all(m.max() < f.c_raw for m in f.comp_lists) and f.grid_of.max() < len(f.comp_lists)


@pytest.mark.parametrize("order", [1, 2, 3, 5, 7, 8])
def test_oracle_cascades_equal_scipy_at_every_order(oracle, order):
    from scipy.signal import sosfilt
    from dss_amd.synthetic import synthetic_ecog
    for fs in (1000, 512):
        f = hc.filters(fs, order)
        x = synthetic_ecog(40 + order, 333, 7, fs=fs)
        for sos, zi in ((f["sos_hg"], f["zi_hg"]), (f["sos_fh"], f["zi_fh"])):
            z0 = np.repeat(zi[:, :, None], 7, axis=2)
            want, zf = sosfilt(np.array(sos), x, axis=0, zi=z0)
            got, zg = oracle.sosfilt(sos, x, z0)
            assert np.array_equal(got, want) and np.array_equal(zg, zf), (fs, order)
            a, z1 = oracle.sosfilt(sos, x[:3], z0)                      # a chunk shorter than the cascade, then the rest
            b, z2 = oracle.sosfilt(sos, x[3:], z1)
            assert np.array_equal(np.concatenate([a, b]), want) and np.array_equal(z2, zf), (fs, order)


@pytest.mark.parametrize("name", hc.NAMES)
def test_oracle_frames_of_every_case(oracle, name):
    """The frame counts of the table are the oracle's, every form a case runs in emits frames, and the step-by-step chain that
    also yields the mean power gives oracle.extractor's own frames."""
    c, x = hc.case(name), hc.signal(name)
    ref = hc.reference(oracle, name)
    assert tuple(a.shape[1] for a in ref["log"]) == c.frames and sum(c.frames) > 0
    assert all(a.shape == (c.S, w, c.C) for a, w in zip(ref["log"], c.frames))
    n_whole = ref["whole_log"].shape[1]
    assert n_whole > 0 and n_whole == hga.trial_frames(sum(c.packets), c.fs, c.wl, c.ws)
    f = hc.filters(c.fs, c.order)
    for s in (0, c.S - 1):
        ex, pos = oracle.extractor(f, c.C, fs=c.fs, wl=c.wl, ws=c.ws), 0
        for k, n in enumerate(c.packets):
            assert np.array_equal(ex.extract(x[s, pos:pos + n]), ref["log"][k][s]), (name, s, k)
            pos += n
        assert np.array_equal(oracle.extractor(f, c.C, fs=c.fs, wl=c.wl, ws=c.ws).extract(x[s]), ref["whole_log"][s])
    assert np.isfinite(ref["whole_power"]).all() and (ref["whole_power"] > 0.01).all()
    assert not np.array_equal(ref["whole_log"][0], ref["whole_log"][c.S - 1])             # the streams differ
    if c.group == "table":
        assert n_whole > hc.WTAB


def test_host_patches_equal_numpy_at_the_new_neighbour_counts():
    patch_list = hc.patches()
    assert [len(nb) for _, nb in patch_list] == list(hc.PATCH_NEIGHBOURS)
    dst = {d for d, _ in patch_list}
    assert all(not dst & set(nb.tolist()) and len(set(nb.tolist())) == len(nb) and nb.max() < hc.PATCH_C for _, nb in patch_list)
    assert [hga.trial_frames(n) for _, n in hc.PATCH_TRIALS] == list(hc.PATCH_FRAMES)
    assert hga.check_trials(hc.PATCH_T, hc.PATCH_TRIALS) == sum(hc.PATCH_FRAMES)
    rng = np.random.default_rng(21)
    for n_rows in (1, 2, 9):
        x = rng.standard_normal((n_rows, hc.PATCH_C)) * 3.0 + 5.0
        got = hga.apply_patches(x, patch_list)
        assert np.array_equal(got, hc.numpy_patch(x, [0, n_rows], patch_list)), n_rows
        for dst_col, nb in patch_list:                                  # one patch at a time: a wrong list cannot hide in another
            want = x.copy()
            want[:, dst_col] = np.mean(x[:, nb], axis=1)
            assert np.array_equal(hga.apply_patches(x, [(dst_col, nb)]), want), (n_rows, len(nb))
    # single-row trials, every neighbour count from 9 to 127: the pairwise rule's block loop and its remainder
    x = rng.standard_normal((1, hc.PATCH_C)) * 3.0 + 5.0
    for k in range(9, 128):
        nb = rng.permutation(np.arange(1, hc.PATCH_C))[:k]
        want = x.copy()
        want[:, 0] = np.mean(x[:, nb], axis=1)
        assert np.array_equal(hga.apply_patches(x, [(0, nb)]), want), k
    with pytest.raises(_lib.DssError, match="1..127 neighbours"):
        hga.apply_patches(x, [(0, np.arange(1, 129))])


@pytest.mark.parametrize("N", hc.STATS_N + hc.STATS_ONE_COLUMN_N)
def test_host_statistics_equal_numpy(N):
    for n_cols in (hc.STATS_C if N in hc.STATS_N else (1,)):
        x = hc.stats_frames(N, n_cols)
        assert np.array_equal(hga.column_stats(x), np.vstack([x.mean(axis=0), x.std(axis=0)])), (N, n_cols)
        assert abs(x[:, -1].mean() - 1e6) < 1.0


def test_one_column_takes_numpys_pairwise_rule():
    """A (N, 1) array is one contiguous run: numpy sums it pairwise, not row by row, and the two differ from 8 rows on."""
    rng = np.random.default_rng(31)
    differs = 0
    for N in list(range(1, 140)) + [255, 256, 257, 1000, 5003]:
        x = rng.standard_normal((N, 1)) * 3.0 + 5.0
        assert np.array_equal(hga.column_stats(x), np.vstack([x.mean(axis=0), x.std(axis=0)])), N
        two = np.hstack([x, x])                                            # the same column beside itself: summed row by row
        assert np.array_equal(hga.column_stats(two), np.vstack([two.mean(axis=0), two.std(axis=0)])), N
        differs += not np.array_equal(hga.column_stats(two)[:, :1], hga.column_stats(x))
    assert differs > 50


def test_front_end_reference_reproduces_the_reference_classes(golden):
    """hc.frontend_reference judges the new layouts on the GPU; here it is held to the two layouts the reference's own classes
    computed: the online chain (129 -> 64, after_select_speech) and the offline one (129 -> 128, after_car)."""
    ec = golden("ecog_chain.npz")
    raw = ec["raw"]
    assert np.array_equal(hc.frontend_reference(raw, *electrodes.reference_frontend()), ec["after_select_speech"])
    assert np.array_equal(hc.frontend_reference(raw, *session.offline_frontend()), ec["after_car"])
    assert np.array_equal(hc.frontend_reference(raw[None], *session.offline_frontend())[0], ec["after_car"])
    # the new layouts: what passes through is the raw column itself, and a repeated source gives a repeated channel
    f = hc.front("front_unreferenced")
    x = hc.front_raw(f.name)
    pre = hc.frontend_reference(x, f.src_col, f.grid_of, f.comp_lists)
    through = np.nonzero(f.grid_of == -1)[0]
    assert np.array_equal(pre[..., through], x[..., f.src_col[through]]) and pre.shape == (1, sum(hc.FRONT_ROWS), f.C)
    f = hc.front("front_repeated_source")
    pre = hc.frontend_reference(hc.front_raw(f.name), f.src_col, f.grid_of, f.comp_lists)
    assert f.grid_of[0] != f.grid_of[f.C - 1] and not np.array_equal(pre[..., 0], pre[..., f.C - 1])
