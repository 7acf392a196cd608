"""The HGA kernels at the shapes of tests/hga_cases.py: filter orders below 8 (lanes without a section), blocks of 16 columns
that span streams, the last ring that fits LDS and the first that does not, windows past the 128-entry table, front ends other
than the reference's two, patches of 1 to 127 neighbours, statistics of 1 to 17 frames and 1 to 130 columns, the largest wire
packets.  Every comparison is array_equal / torch.equal against the oracle, numpy, or the plain path of the same extractor; the
only tolerance is the 1 ulp DESIGN.md states for the device's own log, checked once per group.  tests/test_cpu_hga_cases.py pins
the references used here and proves, without a device, which form each case runs in.

On the tree this file was written against every case passed but one: the statistics of ONE column (C = 1), which numpy sums
pairwise and the library summed row by row; dss_hga_column_stats* follow numpy there now."""
import numpy as np
import pytest

import hga_cases as hc
from dss_amd.synthetic import synthetic_ecog

pytestmark = pytest.mark.gpu


def _extractor(c, path=0):
    from dss_amd.hga import HgaExtractorGPU
    ex = HgaExtractorGPU(c.S, c.C, fs=c.fs, window_length=c.wl, window_shift=c.ws, filters=hc.filter_tuple(c.fs, c.order))
    assert tuple(ex.plan()) == c.plan
    ex._force_path(path)
    return ex


def _paths(c):
    """The default form, and where that is the one-launch kernel the three launches as well."""
    return (0, 2) if c.plan[5] else (0,)


def _packets(c):
    pos = 0
    for k, n in enumerate(c.packets):
        yield k, pos, n
        pos += n


def _same(got, want):
    return got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("name", hc.NAMES)
def test_streaming_forms_equal_the_oracle(oracle, name):
    """Host-buffer path and device-resident mean power, packet by packet with carried state, in every form the case has; a reset
    in mid-sequence and the recording as one chunk; the streams permuted."""
    import torch
    c, x, ref = hc.case(name), hc.signal(name), hc.reference(oracle, name)
    d = torch.from_numpy(x.copy()).cuda()
    seen = {}
    for path in _paths(c):
        ex = _extractor(c, path)
        for k, pos, n in _packets(c):
            assert ex.frames_for(n) == c.frames[k]
            assert _same(ex.extract(x[:, pos:pos + n]), ref["log"][k]), (name, path, k)
        ex.reset()                                              # mid-sequence: the next chunk is a first chunk again
        assert _same(ex.extract(x), ref["whole_log"]), (name, path)
        ex.reset()
        power = []
        for k, pos, n in _packets(c):
            power.append(ex.extract_torch(d[:, pos:pos + n].contiguous(), apply_log=False).cpu().numpy())
            assert _same(power[k], ref["power"][k]), (name, path, k)
        ex.reset()
        assert _same(ex.extract_torch(d, apply_log=False).cpu().numpy(), ref["whole_power"]), (name, path)
        seen[path] = power
    if len(seen) == 2:
        assert all(np.array_equal(a, b) for a, b in zip(seen[0], seen[2]))
    perm = np.roll(np.arange(c.S), 1)
    ex = _extractor(c)
    for k, pos, n in _packets(c):
        assert _same(ex.extract(x[perm][:, pos:pos + n]), ref["log"][k][perm]), (name, k)


@pytest.mark.parametrize("name", [n for n in hc.NAMES if hc.case(n).plan[5]])
def test_trial_list_equals_fresh_extractors(oracle, name):
    """hga_trials_kernel: the recording as one trial is the recording as one chunk into a fresh extractor; a second, shorter
    trial rides in the same list (in beyond_table the first has more than 128 frames); the streaming state is not touched."""
    import torch
    c, x, ref = hc.case(name), hc.signal(name), hc.reference(oracle, name)
    T = x.shape[1]
    a, n = 7, min(T - 7, 2 * c.plan[0] + c.plan[1] + 3)
    ex = _extractor(c)
    first = ex.extract(x[:, :c.packets[0]])                     # a streaming call before: its state must survive the trial calls
    for s in range(c.S):
        short = hc.Chain(oracle, hc.filters(c.fs, c.order), c.C, c.fs, c.wl, c.ws).extract(x[s, a:a + n])
        got = ex.extract_trials(x[s], [(0, T), (a, n)])
        W = ref["whole_log"].shape[1]
        assert len(short[1]) > 0 and got.shape == (W + len(short[1]), c.C)
        assert np.array_equal(got[:W], ref["whole_log"][s]) and np.array_equal(got[W:], short[1]), (name, s)
        power = ex.extract_trials_torch(torch.from_numpy(x[s].copy()).cuda(), [(a, n), (0, T)], apply_log=False).cpu().numpy()
        assert np.array_equal(power[:len(short[0])], short[0]) and np.array_equal(power[len(short[0]):], ref["whole_power"][s])
    assert _same(first, ref["log"][0])
    pos = c.packets[0]
    assert _same(ex.extract(x[:, pos:pos + c.packets[1]]), ref["log"][1])


@pytest.mark.parametrize("name", [n for n in hc.NAMES if not hc.case(n).plan[5]])
def test_first_ring_that_does_not_fit_refuses_a_trial_list(oracle, name):
    from dss_amd import _lib
    c, x, ref = hc.case(name), hc.signal(name), hc.reference(oracle, name)
    ex = _extractor(c)
    assert ex.plan().fused == 0 and ex.plan().ring_bytes == hc.RING_LIMIT + 1024
    k0, pos0, n0 = next(_packets(c))
    assert _same(ex.extract(x[:, pos0:pos0 + n0]), ref["log"][0])
    with pytest.raises(_lib.DssError, match="does not fit"):
        ex.extract_trials(x[0], [(0, x.shape[1])])
    for k, pos, n in list(_packets(c))[1:]:                     # the handle streams on, state intact
        assert _same(ex.extract(x[:, pos:pos + n]), ref["log"][k]), (name, k)


@pytest.mark.parametrize("name", hc.names("tails"))
def test_zscore_epilogue_in_blocks_that_span_streams(oracle, name):
    """Distinct per-channel statistics: a lane that took its channel from the wrong column, or its row from the wrong stream,
    cannot give (frame - mean[c]) / std[c]."""
    import torch
    c, x, ref = hc.case(name), hc.signal(name), hc.reference(oracle, name)
    mean, std = hc.zscore(c.C)
    d = torch.from_numpy(x.copy()).cuda()
    for path in _paths(c):
        ex = _extractor(c, path)
        ex.set_zscore(mean, std)
        for k, pos, n in _packets(c):
            got = ex.extract_torch(d[:, pos:pos + n].contiguous(), apply_log=False).cpu().numpy()
            assert _same(got, (ref["power"][k] - mean) / std), (name, path, k)
        ex.reset()
        for k, pos, n in _packets(c):                           # host-buffer path: glibc log, then the same two operations
            assert _same(ex.extract(x[:, pos:pos + n]), (ref["log"][k] - mean) / std), (name, path, k)
    ex = _extractor(c)
    ex.set_zscore(mean, std)
    got = ex.extract_trials_torch(torch.from_numpy(x[c.S - 1].copy()).cuda(), [(0, x.shape[1])], apply_log=False).cpu().numpy()
    assert _same(got, (ref["whole_power"][c.S - 1] - mean) / std)


@pytest.mark.parametrize("group", hc.GROUPS)
def test_device_log_within_one_ulp(oracle, group):
    """The device-resident log variant (OCML log against glibc's: 1 ulp, DESIGN.md "HGA log"), once per group."""
    import torch
    name = hc.names(group)[0]
    c, x, ref = hc.case(name), hc.signal(name), hc.reference(oracle, name)
    got = _extractor(c).extract_torch(torch.from_numpy(x.copy()).cuda(), apply_log=True).cpu().numpy()
    want = ref["whole_log"]
    assert got.shape == want.shape
    ulp = np.abs(got - want) / np.spacing(np.abs(want))
    print(f"{name}: device log vs glibc, max {ulp.max()} ulp")
    assert ulp.max() <= 1.0


def _front_pair(f, S=1):
    from dss_amd.hga import HgaExtractorGPU
    fe, plain = HgaExtractorGPU(S, f.C), HgaExtractorGPU(S, f.C)
    fe.set_frontend(f.c_raw, f.src_col, f.grid_of, f.comp_lists)
    return fe, plain


@pytest.mark.parametrize("name", hc.FRONT_NAMES)
def test_front_end_layouts(name):
    """extract_raw(raw) is extract(pre) of a plain extractor with pre from the sequential reference, packet by packet with
    carried state: 1, 31, 32, 33 and 100 rows against the kernel's tile of 32 rows."""
    import torch
    f = hc.front(name)
    raw = hc.front_raw(name)
    pre = hc.frontend_reference(raw, f.src_col, f.grid_of, f.comp_lists)
    fe, plain = _front_pair(f)
    pos, frames = 0, 0
    for n in hc.FRONT_ROWS:
        got, want = fe.extract_raw(raw[:, pos:pos + n]), plain.extract(pre[:, pos:pos + n])
        assert _same(got, want) and got.shape[1] > 0, (name, n)
        pos += n
        frames += got.shape[1]
    assert frames == 1 + 3 + 3 + 3 + 10
    # three streams (33, 60 and 120 rows per launch), device-resident: the mean power, exact
    raw3 = hc.front_raw(name, S=3)
    pre3 = hc.frontend_reference(raw3, f.src_col, f.grid_of, f.comp_lists)
    fe, plain = _front_pair(f, S=3)
    d_raw, d_pre = torch.from_numpy(raw3).cuda(), torch.from_numpy(pre3).cuda()
    pos = 0
    for n in (11, 20, 40):
        got = fe.extract_raw_torch(d_raw[:, pos:pos + n].contiguous(), apply_log=False)
        want = plain.extract_torch(d_pre[:, pos:pos + n].contiguous(), apply_log=False)
        assert got.shape == want.shape and torch.equal(got, want), (name, n)
        pos += n


def test_front_end_refusals_leave_the_handle_serviceable():
    from dss_amd import _lib
    from dss_amd.hga import HgaExtractorGPU
    f = hc.front("front_four_grids")
    raw = hc.front_raw(f.name)
    pre = hc.frontend_reference(raw, f.src_col, f.grid_of, f.comp_lists)
    fe, plain = _front_pair(f)
    assert _same(fe.extract_raw(raw[:, :33]), plain.extract(pre[:, :33]))
    with pytest.raises(_lib.DssError, match="at most 4 grids"):            # five grids: refused, the four stay configured
        fe.set_frontend(f.c_raw, f.src_col, f.grid_of, list(f.comp_lists) + [np.array([0, 1])])
    assert fe.c_raw == f.c_raw and _same(fe.extract_raw(raw[:, 33:97]), plain.extract(pre[:, 33:97]))
    # one raw column more than the tile holds: the caller gets the error (from set_frontend or from the first call)
    big = hc.front("front_largest")
    wide = big.c_raw + 1
    ex = HgaExtractorGPU(1, big.C)
    x = np.random.default_rng(5).standard_normal((1, 40, wide))
    with pytest.raises(_lib.DssError, match="exceed the tile"):
        ex.set_frontend(wide, big.src_col, big.grid_of, big.comp_lists)
        ex.extract_raw(x)
    ex.set_frontend(big.c_raw, big.src_col, big.grid_of, big.comp_lists)   # the handle has not moved: a first chunk follows
    plain = HgaExtractorGPU(1, big.C)
    want = plain.extract(hc.frontend_reference(x[..., :big.c_raw], big.src_col, big.grid_of, big.comp_lists))
    assert _same(ex.extract_raw(np.ascontiguousarray(x[..., :big.c_raw])), want) and want.shape[1] == 1


def test_patches_of_1_to_127_neighbours():
    """hga_patch_kernel behind a trial list whose trials emit 1, 1, 2 and 9 frames: numpy's mean of the neighbour columns on the
    device's own unpatched frames, trial by trial (one frame: the pairwise rule, its block loop from 16 and its remainder from 9
    neighbours), then the z-score behind the patch."""
    import torch
    from dss_amd import hga
    ex = hga.HgaExtractorGPU(1, hc.PATCH_C)
    rec = synthetic_ecog(8701, hc.PATCH_T, hc.PATCH_C)
    d = torch.from_numpy(rec).cuda()
    bounds = np.concatenate([[0], np.cumsum(hc.PATCH_FRAMES)])
    patch_list = hc.patches()
    frames = ex.extract_trials_torch(d, hc.PATCH_TRIALS).cpu().numpy()
    assert frames.shape == (bounds[-1], hc.PATCH_C)
    ex.set_patches(patch_list)
    patched = ex.extract_trials_torch(d, hc.PATCH_TRIALS).cpu().numpy()
    want = hc.numpy_patch(frames, bounds, patch_list)
    for (dst, nb), k in zip(patch_list, hc.PATCH_NEIGHBOURS):
        assert np.array_equal(patched[:, dst], want[:, dst]), k
    assert np.array_equal(patched, want)
    assert np.array_equal(patched, np.concatenate([hga.apply_patches(frames[a:b], patch_list) for a, b in zip(bounds, bounds[1:])]))
    rest = np.setdiff1d(np.arange(hc.PATCH_C), [dst for dst, _ in patch_list])
    assert np.array_equal(patched[:, rest], frames[:, rest])
    mean, std = hc.zscore(hc.PATCH_C)
    ex.set_zscore(mean, std)
    assert np.array_equal(ex.extract_trials_torch(d, hc.PATCH_TRIALS).cpu().numpy(), (patched - mean) / std)
    # host-buffer path: the same patch on its own (glibc-log) frames
    ex.set_zscore(None)
    host_patched = ex.extract_trials(rec, hc.PATCH_TRIALS)
    ex.set_patches(None)
    host = ex.extract_trials(rec, hc.PATCH_TRIALS)
    assert np.array_equal(host_patched, hc.numpy_patch(host, bounds, patch_list))


@pytest.mark.parametrize("N", hc.STATS_N + hc.STATS_ONE_COLUMN_N)
def test_device_statistics_equal_numpy(N):
    import torch
    from dss_amd import hga
    for n_cols in (hc.STATS_C if N in hc.STATS_N else (1,)):
        x = hc.stats_frames(N, n_cols)
        got = hga.column_stats_torch(torch.from_numpy(x).cuda()).cpu().numpy()
        assert np.array_equal(got, np.vstack([x.mean(axis=0), x.std(axis=0)])), (N, n_cols)


@pytest.mark.parametrize("n_channels", [64, 129])
def test_wire_packets_at_the_tile(n_channels):
    """hga_wire_kernel's 64 KB tile: the accepted packets of the table equal the parsed-packet path, the refused ones raise, and
    the next ordinary packet is exact."""
    import torch
    from dss_amd import _lib
    from dss_amd.hga import HgaExtractorGPU
    S = 2
    rng = np.random.default_rng(8900 + n_channels)
    a, b = HgaExtractorGPU(S, n_channels), HgaExtractorGPU(S, n_channels)
    steps = [(n, ok) for c, n, ok in hc.WIRE if c == n_channels] + [(40, True)]
    assert [ok for _, ok in steps].count(False) == 1 and steps[-2][1] is False
    frames = 0
    for n, ok in steps:
        assert hc.wire_fits(n_channels, n) == ok
        payload = (rng.standard_normal((S, n_channels, n)) * 40.0).astype(np.float32)
        parsed = np.ascontiguousarray(payload.transpose(0, 2, 1).astype(np.float64))
        if not ok:
            with pytest.raises(_lib.DssError, match="exceeds the 64 KB tile"):
                b.extract_wire_torch(torch.from_numpy(payload).cuda())
            continue
        want = a.extract_torch(torch.from_numpy(parsed).cuda())
        got = b.extract_wire_torch(torch.from_numpy(payload).cuda())
        assert got.shape == want.shape and torch.equal(got, want), (n_channels, n)
        frames += got.shape[1]
    assert frames > 4
