"""The dropout-mask generator of Part 14 of include/dss_hip.h restated in numpy, from the definition alone: a vectorised
Philox4x32-10 (Salmon et al., SC'11) and ``reference_mask``.  The library's kernel and its CPU path are held to this bit for bit."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# (counter, key, block): the known answers of the header
KNOWN_ANSWERS = (
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) of 32-bit words (broadcast against each other) -> blocks (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(MASK32)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(MASK32)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    lo, sh = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2            # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & lo, (p0 >> sh) ^ c3 ^ k1, p0 & lo
        k0, k1 = (k0 + np.uint64(W0)) & lo, (k1 + np.uint64(W1)) & lo
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def scale_of(p):
    """float32 1 / (1 - p): 1.0 - p in double, rounded to float32, then one float32 division."""
    return np.float32(1.0) / np.float32(1.0 - p)


def words(n, seed, draw):
    """The first n 32-bit words of the stream (seed, draw): word e is word e & 3 of block e >> 2."""
    seed, draw = int(seed), int(draw)
    b = np.arange((n + 3) // 4, dtype=np.uint64)
    counter = np.stack([b & np.uint64(MASK32), b >> np.uint64(32), np.full_like(b, draw & MASK32), np.full_like(b, draw >> 32)], axis=-1)
    return philox4x32_10(counter, np.array([seed & MASK32, seed >> 32], dtype=np.uint64)).reshape(-1)[:n]


def reference_mask(rows, width, seed, draw, p):
    """(rows, width) float32: scale where u >= float32(p), else 0, with u = float32(word >> 8) * 2^-24."""
    u = (words(rows * width, seed, draw) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.where(u >= np.float32(p), scale_of(p), np.float32(0.0)).astype(np.float32).reshape(rows, width)
