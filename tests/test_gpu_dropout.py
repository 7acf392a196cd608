"""The dropout masks drawn on the device (csrc/dropout.hip, Part 14 of include/dss_hip.h) against the numpy restatement of their
definition (tests/philox_reference.py), bit for bit, and through the three trainers: a trainer given a ``DeviceMaskSource``
computes the bits of the same trainer given ``reference_mask`` arrays, so no new tolerance is needed -- the host-mask path is pinned
to float64 autograd by tests/test_gpu_*_training.py and test_gpu_decoder_group.py.

Every mask of the kernel tests lies in an arena between 64 sentinel floats (a NaN bit pattern) on either side, and the whole arena
is compared: sentinels, padding and the buffers of empty entries must come back untouched."""
import functools

import numpy as np
import pytest

import decoder_training_reference as D
import lstm_reference as R
import philox_reference as P
import vad_training_reference as V

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD             # a quiet NaN no mask holds
GUARD = 64
SHAPES = ((1, 1), (1, 3), (3, 5), (7, 33), (1, 4), (65, 256), (130, 200), (300, 200))
PS = (0.5, 0.1, 0.999)
SEEDS = (0, 1234, 2 ** 63 + 5)
DRAWS = (0, 7, 2 ** 32 + 3)


@pytest.fixture(scope="module")
def T():
    from dss_amd import training
    return training


@pytest.fixture(scope="module")
def L():
    from dss_amd import _lib
    return _lib.load()


reference = functools.lru_cache(maxsize=None)(P.reference_mask)     # computed once per case, shared, never written to


class Arena:
    """One device buffer of slots [64 sentinels | ``offset`` sentinels | rows * width payload | sentinels up to a multiple of 4 |
    64 sentinels], all sentinels at first.  Slots start at multiples of 4 floats of a 256-byte aligned base, so a payload is
    ``offset`` floats past a 16-byte boundary."""

    def __init__(self, sizes, offsets=None):
        import torch
        offsets = [0] * len(sizes) if offsets is None else offsets
        self.payload, total = [], 0
        for n, off in zip(sizes, offsets):
            self.payload.append((total + GUARD + off, n))
            total += -(-(2 * GUARD + off + n) // 4) * 4
        self.t = torch.full((total,), SENTINEL, dtype=torch.int32, device="cuda")
        assert self.t.data_ptr() % 256 == 0

    def ptr(self, i):
        return self.t.data_ptr() + 4 * self.payload[i][0]

    def assert_holds(self, masks, what=""):
        """masks[i]: the float32 array slot i must hold, or None: untouched.  Everything else: sentinels."""
        want = np.full(self.t.numel(), SENTINEL, np.int32)
        for (a, n), m in zip(self.payload, masks):
            if m is not None:
                assert m.size == n and m.dtype == np.float32
                want[a:a + n] = m.reshape(-1).view(np.int32)
        got = self.t.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            slot = [i for i, (a, n) in enumerate(self.payload) if a - GUARD <= bad[0]][-1]
            raise AssertionError(f"{what}: {len(bad)} words differ, the first at float {bad[0]} (slot {slot}, payload at {self.payload[slot][0]})")


def _entry(T, ptr, rows, width, seed, draw, p):
    return T._DropoutEntry(ptr, rows, width, seed, draw, p, float(P.scale_of(p)))


def _launch(L, T, entries):
    import torch
    rc = L.dss_dropout_masks_dev((T._DropoutEntry * len(entries))(*entries), len(entries), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.dss_last_error().decode()


# ---- the kernel against the definition -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_reference(L, T, shape):
    rows, width = shape
    cases = [(p, seed, draw) for p in PS for seed in SEEDS for draw in DRAWS]
    arena = Arena([rows * width] * len(cases))
    for i, (p, seed, draw) in enumerate(cases):
        _launch(L, T, [_entry(T, arena.ptr(i), rows, width, seed, draw, p)])
    arena.assert_holds([reference(rows, width, seed, draw, p) for p, seed, draw in cases], str(shape))


@pytest.mark.parametrize("shape", ((7, 33), (130, 200)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_masks_that_start_off_a_16_byte_boundary(L, T, shape):
    rows, width = shape
    arena = Arena([rows * width] * 4, offsets=[0, 1, 2, 3])
    assert [arena.ptr(i) % 16 for i in range(4)] == [0, 4, 8, 12]
    _launch(L, T, [_entry(T, arena.ptr(i), rows, width, 1234, 7, 0.5) for i in range(4)])
    arena.assert_holds([reference(rows, width, 1234, 7, 0.5)] * 4, str(shape))


def _table64():
    """64 entries of mixed shapes: rows 0 .. 300, nine of them empty (three of those with a null pointer), seeds and draws all
    distinct, the three probabilities in turn.  [(rows, width, seed, draw, p)]"""
    rng = np.random.default_rng(6464)
    rows = rng.integers(1, 301, 64)
    rows[[0, 5, 17, 18, 31, 40, 52, 62, 63]] = 0
    rows[[1, 2]] = (300, 1)
    widths = rng.choice([1, 3, 4, 33, 200, 256], 64)
    return [(int(r), int(w), 1000 + 7 * i + (2 ** 63 if i % 5 == 0 else 0), 3 * i + (2 ** 32 if i % 4 == 1 else 0), PS[i % 3])
            for i, (r, w) in enumerate(zip(rows, widths))]


def test_sixty_four_entries_in_one_launch_whatever_their_order(L, T):
    table = _table64()
    assert sum(r == 0 for r, *_ in table) == 9 and len({(s, d) for _, _, s, d, _ in table}) == 64
    null = {0, 31, 63}
    want = [None if r == 0 else reference(r, w, s, d, p) for r, w, s, d, p in table]
    sizes = [r * w if r else 40 for r, w, *_ in table]                    # an empty entry's buffer: 40 floats that must stay
    one = Arena(sizes)
    _launch(L, T, [_entry(T, None if i in null else one.ptr(i), *e) for i, e in enumerate(table)])
    one.assert_holds(want, "one launch")
    order = np.random.default_rng(1).permutation(64)
    assert list(order) != sorted(order)
    other = Arena(sizes)
    _launch(L, T, [_entry(T, None if i in null else other.ptr(i), *table[i]) for i in order])
    other.assert_holds(want, "permuted")
    alone = Arena(sizes)
    for i, e in enumerate(table):
        if e[0]:
            _launch(L, T, [_entry(T, alone.ptr(i), *e)])
    alone.assert_holds(want, "one entry per launch")


def test_device_path_equals_the_library_cpu_path(L, T):
    table = _table64()
    arena = Arena([r * w for r, w, *_ in table])
    _launch(L, T, [_entry(T, arena.ptr(i), *e) for i, e in enumerate(table)])
    host = [np.full(r * w, np.float32(np.nan), np.float32) for r, w, *_ in table]
    entries = [_entry(T, h.ctypes.data if h.size else None, *e) for h, e in zip(host, table)]
    assert L.dss_dropout_masks_host((T._DropoutEntry * 64)(*entries), 64) == 0, L.dss_last_error().decode()
    arena.assert_holds([h if h.size else None for h in host], "device against dss_dropout_masks_host")


def test_launches_enqueued_back_to_back(L, T):
    """Eight launches of different tables into eight buffers with nothing between them that waits for the device."""
    import torch
    tables = [[(1 + (37 * k + 11 * i) % 150, (3, 200, 33)[(k + i) % 3], 50 + k, 100 * k + i, PS[(k + i) % 3]) for i in range(1 + k % 3)]
              for k in range(8)]
    arenas = [Arena([r * w for r, w, *_ in tab]) for tab in tables]
    torch.cuda.synchronize()
    for tab, arena in zip(tables, arenas):
        _launch(L, T, [_entry(T, arena.ptr(i), *e) for i, e in enumerate(tab)])
    for k, (tab, arena) in enumerate(zip(tables, arenas)):
        arena.assert_holds([reference(*e) for e in tab], f"launch {k}")


def test_refused_before_any_launch(L, T):
    arena = Arena([15, 15])
    good = _entry(T, arena.ptr(0), 3, 5, 1, 2, 0.5)
    for bad in (_entry(T, arena.ptr(1) + 2, 3, 5, 1, 2, 0.5), _entry(T, arena.ptr(1), 3, 5, 1, 2, 1.5), _entry(T, None, 3, 5, 1, 2, 0.5),
                _entry(T, arena.ptr(1), 3, -5, 1, 2, 0.5)):
        assert L.dss_dropout_masks_dev((T._DropoutEntry * 2)(good, bad), 2, None) == -1
    assert L.dss_dropout_masks_dev((T._DropoutEntry * 2)(_entry(T, None, 0, 5, 1, 2, 0.5), _entry(T, None, 0, 5, 1, 2, 0.5)), 2, None) == -1
    arena.assert_holds([None, None], "refused calls")


def test_device_mask_source_on_the_device(T):
    import torch
    src = T.DeviceMaskSource(2 ** 63 + 5)
    a = src.mask(7, 33, 0.1)
    assert a.is_cuda and a.dtype == torch.float32 and src.draw == 1
    assert np.array_equal(a.cpu().numpy(), reference(7, 33, 2 ** 63 + 5, 0, 0.1))
    got = src.masks([(130, 200), None, (3, 5), (0, 4), (1, 1)], 0.5)
    assert src.draw == 5 and got[1] is None and tuple(got[3].shape) == (0, 4)
    for g, shape, draw in ((got[0], (130, 200), 1), (got[2], (3, 5), 2), (got[4], (1, 1), 4)):
        assert g.data_ptr() % 16 == 0 and np.array_equal(g.cpu().numpy(), reference(*shape, 2 ** 63 + 5, draw, 0.5))
    out = torch.zeros((3, 5), device="cuda")
    src.draw = 2
    assert src.mask(3, 5, 0.5, out=out) is out and torch.equal(out, got[2])
    T.device_dropout_masks([(out, 9, 8, 0.999), (torch.empty((0, 5), device="cuda"), 1, 1, 0.5)])
    assert np.array_equal(out.cpu().numpy(), reference(3, 5, 9, 8, 0.999))


# ---- through the trainers --------------------------------------------------------------------------------------------------------

O = 20


def _x(x):
    import torch
    return torch.from_numpy(x.astype(np.float32))


def _dec_trial(H, C, n, seed):
    x = R.frames("x2", 1, n, C, 7700 + seed)[0]
    return x, np.random.default_rng(7800 + seed).standard_normal((n, O)).astype(np.float32)


def _assert_same_trainer(a, b, what=""):
    for name, u, v in (("parameters", a.state_dict(), b.state_dict()), ("gradients", a.gradients(), b.gradients()),
                       ("square averages", a.square_avg(), b.square_avg())):
        for k in D.KEYS:
            assert np.array_equal(np.asarray(u[k]), np.asarray(v[k])), (what, name, k)
    assert np.array_equal(a.features(), b.features()), (what, "features")


def test_decoder_trainer_with_a_device_mask_source(T):
    H, C, n, seed = 16, 8, 90, 41
    sd = R.decoder_state_dict(H, C, 1)
    a, b = T.DecoderTrainerGPU(sd, max_frames=n), T.DecoderTrainerGPU(sd, max_frames=n)
    src = T.DeviceMaskSource(seed)
    for k in range(2):
        x, y = _dec_trial(H, C, n, k)
        got = a.train_trial(_x(x), y, dropout=0.5, generator=src, lr=1e-3)
        want = b.trial(_x(x), y, mask=reference(n, 2 * H, seed, k, 0.5), lr=1e-3)
        assert got == want and src.draw == k + 1, (k, got, want)
        _assert_same_trainer(a, b, f"trial {k}")
    assert T.DeviceMaskSource(seed + 1).mask(n, 2 * H, 0.5).cpu().numpy().tobytes() != reference(n, 2 * H, seed, 0, 0.5).tobytes()


def test_vad_trainer_with_a_device_mask_source(T):
    H, C, n, seed = 12, 8, 130, 43
    sd = R.vad_state_dict(H, C, 1)
    a, b = T.VadTrainerGPU(sd, max_window=50), T.VadTrainerGPU(sd, max_window=50)
    src = T.DeviceMaskSource(seed)
    for k in range(2):
        x = R.frames("x2", 1, n, C, 7900 + k)[0]
        y = (np.random.default_rng(7950 + k).random(n) < 0.4).astype(np.uint8)
        got = a.train_trial(x, y, window=50, dropout=0.5, generator=src, lr=1e-3)
        want = b.train_trial(x, y, window=50, masks=reference(n, H, seed, k, 0.5), lr=1e-3)
        assert got.shape == (3,) and np.array_equal(got, want) and src.draw == k + 1, (k, got, want)
        sa, sb = a.state_dict(), b.state_dict()
        assert all(np.array_equal(sa[q].numpy(), sb[q].numpy()) for q in V.KEYS), k


def test_group_epoch_with_device_masks_is_three_single_trainers(T):
    """M = 3 with 3, 1 and 2 trials per epoch, so models 1 and 2 sit out the later steps; two epochs, so the draws run on."""
    import torch
    H, C, seeds, n_trials = 16, 8, (5, 2 ** 63 + 6, 7), (3, 1, 2)
    sds = [R.decoder_state_dict(H, C, s) for s in (1, 2, 1)]
    trials = [[_dec_trial(H, C, 20 + 9 * ((m + 2 * k) % 4), 10 * m + k) for k in range(n)] for m, n in enumerate(n_trials)]
    lengths = [[len(x) for x, _ in t] for t in trials]
    g = T.DecoderGroupTrainerGPU(sds, max_frames=64)
    singles = [T.DecoderTrainerGPU(sd, max_frames=64) for sd in sds]
    srcs = [T.DeviceMaskSource(s) for s in seeds]
    gens = [torch.Generator().manual_seed(1) for _ in seeds]
    seen = []

    def step(ks, masks):
        assert all((k is None) == (m is None) for k, m in zip(ks, masks)) and all(m is None or (m.is_cuda and m.data_ptr() % 16 == 0) for m in masks)
        seen.append([None if m is None else m.cpu().numpy() for m in masks])
        return g.step([None if k is None else _x(trials[m][k][0]) for m, k in enumerate(ks)],
                      [None if k is None else trials[m][k][1] for m, k in enumerate(ks)], masks, lr=1e-3)

    for epoch in range(2):
        steps, losses = T._group_epoch(step, gens, n_trials, lengths, H, 0.5, False, sources=srcs)
        assert steps == [[0, 0, 0], [1, None, 1], [2, None, None]]
        losses = torch.stack(losses).cpu().numpy()
        for m in range(3):
            for k in range(n_trials[m]):
                draw = epoch * n_trials[m] + k
                mask = reference(lengths[m][k], 2 * H, seeds[m], draw, 0.5)
                assert np.array_equal(seen[3 * epoch + k][m], mask), (epoch, m, k)
                assert losses[k, m] == singles[m].trial(_x(trials[m][k][0]), trials[m][k][1], mask=mask, lr=1e-3), (epoch, m, k)
    assert [s.draw for s in srcs] == [6, 2, 4]
    for m in range(3):
        for name, u, v in (("parameters", g.state_dict(m), singles[m].state_dict()), ("gradients", g.gradients(m), singles[m].gradients()),
                           ("square averages", g.square_avg(m), singles[m].square_avg())):
            assert all(np.array_equal(np.asarray(u[k]), np.asarray(v[k])) for k in D.KEYS), (m, name)
        assert np.array_equal(g.features(m), singles[m].features()), m


@pytest.fixture(scope="module")
def corpora():
    """Three corpora of 4, 6 and 5 trials of 60 .. 140 frames (C 8, 20 targets), and the weights of three decoders (H 16)."""
    rng = np.random.default_rng(515)
    out = []
    for m, n_trials in enumerate((4, 6, 5)):
        lens = rng.integers(60, 141, n_trials)
        x = rng.standard_normal((int(lens.sum()), 8)).astype(np.float32)
        y = rng.standard_normal((int(lens.sum()), O)).astype(np.float32)
        out.append(dict(hga_activity=x, lpc_coefficients=y, trial_ids=np.concatenate([np.full(n, k) for k, n in enumerate(lens)])))
    return out, [R.decoder_state_dict(16, 8, s) for s in (1, 1, 2)]


def _same_run(a, b):
    return a[1] == b[1] and all(np.array_equal(a[0][k].numpy(), b[0][k].numpy()) for k in D.KEYS)


def test_train_decoders_with_device_masks_is_train_decoder_per_model(T, corpora):
    cs, sds = corpora
    seeds = [5, 6, 7]
    got = T.train_decoders(sds, cs, cs, epochs=2, lr=1e-3, seeds=seeds, mask_source="device")
    host = T.train_decoders(sds, cs, cs, epochs=2, lr=1e-3, seeds=seeds)
    for m in range(3):
        alone = T.train_decoder(sds[m], cs[m], cs[m], epochs=2, lr=1e-3, seed=seeds[m], mask_source="device")
        assert got[m][1] == alone[1], (m, got[m][1], alone[1])
        assert [h["update_steps"] for h in alone[1]] == [(4, 6, 5)[m] * (e + 1) for e in range(2)]
        assert _same_run(got[m], alone), m
        assert got[m][1] != host[m][1], m                                  # another random stream than the host generator's


def test_the_default_is_the_host_generator(T, corpora):
    cs, sds = corpora
    a = T.train_decoder(sds[0], cs[0], cs[0], epochs=1, lr=1e-3, seed=3)
    assert _same_run(a, T.train_decoder(sds[0], cs[0], cs[0], epochs=1, lr=1e-3, seed=3, mask_source="host"))
    b = T.train_decoders(sds[:2], cs[:2], cs[:2], epochs=1, lr=1e-3, seeds=[3, 4])
    c = T.train_decoders(sds[:2], cs[:2], cs[:2], epochs=1, lr=1e-3, seeds=[3, 4], mask_source="host")
    assert all(_same_run(b[m], c[m]) for m in range(2)) and _same_run(a, b[0])
    with pytest.raises(ValueError, match="mask_source"):
        T.train_decoder(sds[0], cs[0], cs[0], epochs=1, mask_source="philox")


def test_train_vad_with_device_masks_is_reproducible(T):
    sd, _, corpus = V.learning_problem()
    lr = V.LEARN["lr"]
    b1, h1 = T.train_vad(sd, corpus, corpus, epochs=1, lr=lr, seed=5, mask_source="device")
    b2, h2 = T.train_vad(sd, corpus, corpus, epochs=1, lr=lr, seed=5, mask_source="device")
    assert h1 == h2 and all(np.array_equal(b1[k].numpy(), b2[k].numpy()) for k in V.KEYS)
    assert np.isfinite(h1[0]["train_loss"]) and h1[0]["update_steps"] > 0
    _, h3 = T.train_vad(sd, corpus, corpus, epochs=1, lr=lr, seed=6, mask_source="device")
    assert h3[0]["train_loss"] != h1[0]["train_loss"]
    _, h4 = T.train_vad(sd, corpus, corpus, epochs=1, lr=lr, seed=5)
    assert h4[0]["train_loss"] != h1[0]["train_loss"]                      # the default: the host generator's stream
