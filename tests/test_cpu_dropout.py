"""The dropout-mask generator of Part 14 without a GPU: the definition's known answers through the numpy restatement
(tests/philox_reference.py) and through the library; ``dss_dropout_masks_host`` against ``reference_mask`` bit for bit; the keep
share of the stream; every refusal of ``dss_dropout_check``; ``DeviceMaskSource``'s bookkeeping."""
import ctypes as C
import math

import numpy as np
import pytest

import philox_reference as P

SHAPES = ((1, 1), (3, 5), (7, 33), (50, 150))
PS = (0.5, 0.1, 0.999)
SEEDS = (0, 1234, 2 ** 63 + 5)
DRAWS = (0, 7, 2 ** 32 + 3)
NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def L():
    from dss_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def T():
    from dss_amd import training
    return training


def _entry(T, buf, rows, width, seed, draw, p, scale=None, offset=0):
    """An entry over a float32 numpy buffer (or a raw address), starting ``offset`` floats in."""
    ptr = buf if isinstance(buf, int) or buf is None else buf.ctypes.data + 4 * offset
    return T._DropoutEntry(ptr, rows, width, seed, draw, p, float(P.scale_of(p)) if scale is None else scale)


def _host_mask(L, T, rows, width, seed, draw, p):
    out = np.full(rows * width, NAN, np.float32)
    assert L.dss_dropout_masks_host((T._DropoutEntry * 1)(_entry(T, out, rows, width, seed, draw, p)), 1) == 0, L.dss_last_error()
    return out.reshape(rows, width)


# ---- the block function ----------------------------------------------------------------------------------------------------------

def test_known_answers_numpy():
    for counter, key, want in P.KNOWN_ANSWERS:
        got = P.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
        assert [int(w) for w in got] == list(want), [hex(int(w)) for w in got]


def test_known_answers_library_block(L):
    for counter, key, want in P.KNOWN_ANSWERS:
        out = (C.c_uint * 4)()
        assert L.dss_selftest_philox((C.c_uint * 4)(*counter), (C.c_uint * 2)(*key), out) == 0
        assert list(out) == list(want), [hex(w) for w in out]
    assert L.dss_selftest_philox(None, None, None) == -1


def test_known_answer_through_a_one_block_mask(L, T):
    """Seed 0 and draw 0 put the all-zero counter and key under a (1, 4) mask: its elements are words 0 .. 3 of the first known
    answer.  Element j is kept at p = u_j and dropped at the next float32 above, which pins the 24 bits of every word that a mask
    uses; a seed and a draw that spell the third answer's key and counter words 2, 3 give another block."""
    want = P.KNOWN_ANSWERS[0][2]
    for j, w in enumerate(want):
        u = np.float32(w >> 8) * np.float32(2.0 ** -24)
        above = np.nextafter(u, np.float32(1.0), dtype=np.float32)
        at, over = _host_mask(L, T, 1, 4, 0, 0, float(u)), _host_mask(L, T, 1, 4, 0, 0, float(above))
        assert at[0, j] == P.scale_of(float(u)) and over[0, j] == 0.0, (j, hex(w))
    (_, _, c2, c3), (k0, k1), _ = P.KNOWN_ANSWERS[2]
    seed, draw = k0 | (k1 << 32), c2 | (c3 << 32)
    block = P.philox4x32_10(np.array([0, 0, c2, c3], np.uint64), np.array([k0, k1], np.uint64))
    u = (block >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(_host_mask(L, T, 1, 4, seed, draw, 0.5)[0], np.where(u >= np.float32(0.5), np.float32(2.0), np.float32(0.0)))


# ---- the library's CPU path against the numpy restatement ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def references():
    """reference_mask of every case, computed once: {(shape, p, seed, draw): mask}."""
    return {(s, p, seed, draw): P.reference_mask(s[0], s[1], seed, draw, p) for s in SHAPES for p in PS for seed in SEEDS for draw in DRAWS}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_masks_equal_the_reference(L, T, references, shape):
    rows, width = shape
    for p in PS:
        scale = P.scale_of(p)
        for seed in SEEDS:
            for draw in DRAWS:
                got = _host_mask(L, T, rows, width, seed, draw, p)
                want = references[(shape, p, seed, draw)]
                assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shape, p, seed, draw)
                assert np.isin(got, (np.float32(0.0), scale)).all()
    assert P.scale_of(0.5) == np.float32(2.0) and T.dropout_scale(0.5) == np.float32(2.0)
    for p in PS:
        assert T.dropout_scale(p).tobytes() == P.scale_of(p).tobytes()


def test_the_high_word_of_the_draw_counts(L, T, references):
    a = references[((50, 150), 0.5, 1234, 2 ** 32 + 3)]
    b = P.reference_mask(50, 150, 1234, 3, 0.5)
    assert not np.array_equal(a, b)
    assert np.array_equal(_host_mask(L, T, 50, 150, 1234, 3, 0.5), b)
    # ... and so do the seed's: three seeds, three masks
    assert len({references[((50, 150), 0.5, s, 7)].tobytes() for s in SEEDS}) == 3


def test_several_entries_and_empty_ones(L, T):
    """One call, five entries, two of them empty (a null pointer and a buffer that must stay as it was)."""
    bufs = [np.full(3 * 5, NAN, np.float32), None, np.full(7 * 33, NAN, np.float32), np.full(8, NAN, np.float32), np.full(4, NAN, np.float32)]
    table = (T._DropoutEntry * 5)(_entry(T, bufs[0], 3, 5, 11, 0, 0.5), _entry(T, None, 0, 9, 12, 1, 0.5), _entry(T, bufs[2], 7, 33, 13, 2, 0.1),
                                  _entry(T, bufs[3], 0, 8, 14, 3, float("nan")), _entry(T, bufs[4], 1, 4, 15, 4, 0.999))
    assert L.dss_dropout_masks_host(table, 5) == 0, L.dss_last_error()
    assert np.array_equal(bufs[0].reshape(3, 5), P.reference_mask(3, 5, 11, 0, 0.5))
    assert np.array_equal(bufs[2].reshape(7, 33), P.reference_mask(7, 33, 13, 2, 0.1))
    assert np.array_equal(bufs[4].reshape(1, 4), P.reference_mask(1, 4, 15, 4, 0.999))
    assert np.isnan(bufs[3]).all()


def test_keep_share_of_the_reference():
    """65 536 blocks at seed 1234, draw 7, p = 0.5: the share of kept elements within 6 binomial standard deviations of 1 - p."""
    n, p = 4 * 65536, 0.5
    kept = float((P.reference_mask(1, n, 1234, 7, p) != 0).mean())
    bound = 6.0 * math.sqrt(p * (1.0 - p) / n)
    print(f"keep share {kept:.5f} over {n} elements: {abs(kept - (1 - p)) / (bound / 6):.2f} sigma (bound +- {bound:.4f})")
    assert bound == pytest.approx(0.0059, abs=5e-5)
    assert abs(kept - (1.0 - p)) <= bound


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_of_the_check(L, T):
    buf = np.full(64, NAN, np.float32)
    good = lambda: _entry(T, buf, 3, 5, 1, 2, 0.5)                                  # noqa: E731

    def refused(entries, n=None, word=None):
        n = len(entries) if n is None else n
        table = (T._DropoutEntry * max(1, len(entries)))(*entries)
        for fn in (L.dss_dropout_check, lambda k, t: L.dss_dropout_masks_host(t, k), lambda k, t: L.dss_dropout_masks_dev(t, k, None)):
            assert fn(n, table) == -1, (n, word)
            assert word is None or word in L.dss_last_error().decode(), (word, L.dss_last_error())

    assert L.dss_dropout_check(1, (T._DropoutEntry * 1)(good())) == 0
    assert L.dss_dropout_check(64, (T._DropoutEntry * 64)(*[good()] * 64)) == 0
    refused([good()], 0, "0 entries")
    refused([good()] * 65, 65, "65 entries")
    refused([good()], -1, "entries")
    assert L.dss_dropout_check(1, None) == -1
    refused([_entry(T, None, 3, 5, 1, 2, 0.5)], word="null")
    refused([good(), _entry(T, buf.ctypes.data + 2, 3, 5, 1, 2, 0.5)], word="entry 1")
    refused([_entry(T, buf, -1, 5, 1, 2, 0.5)], word="negative")
    refused([_entry(T, buf, 3, -5, 1, 2, 0.5)], word="negative")
    refused([_entry(T, buf, 0, -5, 1, 2, 0.5)], word="negative")
    refused([_entry(T, buf, 1 << 16, 1 << 15, 1, 2, 0.5)], word="2^31")
    refused([_entry(T, buf, 46341, 46341, 1, 2, 0.5)], word="2^31")
    for p in (0.0, 1.0, -0.25, 1.5, float("nan"), float("inf")):
        refused([good(), _entry(T, buf, 3, 5, 1, 2, p, scale=2.0)], word="(0, 1)")
    for scale in (0.0, -2.0, float("nan"), float("inf")):
        refused([_entry(T, buf, 3, 5, 1, 2, 0.5, scale=scale)], word="scale")
    refused([_entry(T, None, 0, 5, 1, 2, 0.5), _entry(T, buf, 4, 0, 1, 2, 0.5)], word="empty")
    assert np.isnan(buf).all()                                                      # nothing was written by any of them
    # the largest mask the check lets through is not filled here: only checked
    assert L.dss_dropout_check(1, (T._DropoutEntry * 1)(_entry(T, buf, 1 << 15, (1 << 16) - 1, 1, 2, 0.5))) == 0
    assert C.sizeof(T._DropoutEntry) == 40


# ---- DeviceMaskSource ------------------------------------------------------------------------------------------------------------

def test_device_mask_source_bookkeeping(T):
    src = T.DeviceMaskSource(1234, device="cpu")
    assert (src.seed, src.draw) == (1234, 0)
    a = src.mask(3, 5, 0.5)
    assert src.draw == 1 and np.array_equal(a.numpy(), P.reference_mask(3, 5, 1234, 0, 0.5))
    assert src.mask(3, 5, 0.0) is None and src.draw == 1                            # p == 0: no mask, nothing drawn
    got = src.masks([(7, 33), None, (2, 2), None, (1, 1)], 0.1)
    assert src.draw == 4 and got[1] is None and got[3] is None
    for g, (shape, draw) in zip((got[0], got[2], got[4]), (((7, 33), 1), ((2, 2), 2), ((1, 1), 3))):
        assert tuple(g.shape) == shape and np.array_equal(g.numpy(), P.reference_mask(*shape, 1234, draw, 0.1))
        assert g.data_ptr() % 16 == got[0].data_ptr() % 16                          # packed at multiples of 4 floats
    assert src.masks([(2, 2), None], 0.0) == [None, None] and src.draw == 4
    assert src.masks([None, None], 0.5) == [None, None] and src.draw == 4
    src.draw = 2 ** 32 + 3                                                          # settable: a mask can be drawn again, a run resumed
    import torch
    out = torch.full((4, 6), float("nan"))
    assert src.mask(4, 6, 0.999, out=out) is out and src.draw == 2 ** 32 + 4
    assert np.array_equal(out.numpy(), P.reference_mask(4, 6, 1234, 2 ** 32 + 3, 0.999))
    more = src.masks([(1, 3)] * 70, 0.5)                                            # more than one call's 64 entries
    assert src.draw == 2 ** 32 + 74
    assert all(np.array_equal(m.numpy(), P.reference_mask(1, 3, 1234, 2 ** 32 + 4 + i, 0.5)) for i, m in enumerate(more))
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            T.DeviceMaskSource(bad)
    with pytest.raises(ValueError):
        src.draw = -1
    for p in (1.0, -0.1):
        with pytest.raises(ValueError, match="dropout must be in"):
            src.mask(2, 2, p)
    with pytest.raises(ValueError, match="out must be"):
        src.mask(2, 2, 0.5, out=torch.zeros(2, 3))
    assert src.draw == 2 ** 32 + 74                                                 # a refused call draws nothing
    big = T.DeviceMaskSource(2 ** 63 + 5, device="cpu")
    big.draw = 7
    assert np.array_equal(T.dropout_mask(5, 9, 0.5, big).numpy(), P.reference_mask(5, 9, 2 ** 63 + 5, 7, 0.5)) and big.draw == 8
    assert np.array_equal(T.decoder_dropout_mask(5, 9, 0.5, big).numpy(), P.reference_mask(5, 18, 2 ** 63 + 5, 8, 0.5)) and big.draw == 9


def test_the_host_generator_path_is_untouched(T):
    """``dropout_mask`` with a torch.Generator: torch.rand >= p over 1 - p, as before this part existed."""
    import torch
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    want = (torch.rand((6, 10), generator=g2, dtype=torch.float32) >= 0.5).to(torch.float32) / np.float32(0.5)
    assert torch.equal(T.dropout_mask(6, 10, 0.5, g1), want)
    for fn in (T.train_vad, T.train_decoder, T.train_decoders):
        with pytest.raises(ValueError, match="mask_source"):
            fn(None, None, None, mask_source="gpu") if fn is not T.train_decoders else fn([], [], [], mask_source="gpu")
