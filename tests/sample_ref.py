"""The model of agx_ntt_sample_uniform / _ternary / _cbd in Python integers, from the definition in include/agx_ntt.h and nothing of the library: the ChaCha20
block function of RFC 8439 section 2.3 (20 rounds) and the three ways its 64-bit candidates become coefficients.  tests/test_sample_reference.py judges it on
the CPU (the RFC's vectors, the properties of the definition); tests/test_gpu_sample.py compares the device with it word for word."""
import functools

import numpy as np

M32 = 0xFFFFFFFF
CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
SMALL_TAG = 0xFFFF
MAX_BLOCKS = 16


def _rotl(x, k):
    return ((x << k) | (x >> (32 - k))) & M32


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & M32
    x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32
    x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32
    x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32
    x[b] = _rotl(x[b] ^ x[c], 7)


def block(key, w12, w13, w14, w15):
    """o[0..15]: state words 0..3 the constants, 4..11 the 32 key bytes as little-endian words, 12..15 as given"""
    key = bytes(key)
    assert len(key) == 32
    s = list(CONSTANTS) + [int.from_bytes(key[4 * i:4 * i + 4], "little") for i in range(8)] + [w12 & M32, w13 & M32, w14 & M32, w15 & M32]
    x = list(s)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12), _quarter(x, 1, 5, 9, 13), _quarter(x, 2, 6, 10, 14), _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15), _quarter(x, 1, 6, 11, 12), _quarter(x, 2, 7, 8, 13), _quarter(x, 3, 4, 9, 14)
    return [(a + b) & M32 for a, b in zip(x, s)]


def keystream(o):
    """the 64 bytes of a block: its words, little-endian"""
    return b"".join(w.to_bytes(4, "little") for w in o)


@functools.lru_cache(maxsize=1 << 16)
def candidates(key, nonce, tag, frame, cell, k):
    """the eight 64-bit candidates of block k of a cell (kept: the tests ask for the same cells under several moduli and widths)"""
    assert 0 <= tag <= 0xFFFF and 0 <= cell < 4096 and 0 <= k < 16 and 0 <= frame < 1 << 32 and 0 <= nonce < 1 << 64
    o = block(key, tag << 16 | cell << 4 | k, frame, nonce & M32, nonce >> 32)
    return tuple(o[2 * i] | o[2 * i + 1] << 32 for i in range(8))


def uniform_cell(key, nonce, prime, frame, cell, q, W):
    """(the W words of the cell, the blocks it read)"""
    mask = (1 << int(q).bit_length()) - 1
    out = []
    for k in range(MAX_BLOCKS):
        for c in candidates(key, nonce, prime, frame, cell, k):
            if c & mask < q and len(out) < W:
                out.append(c & mask)
        if len(out) == W:
            return out, k + 1
    return out + [0] * (W - len(out)), MAX_BLOCKS


def ternary_value(w):
    for r in range(32):
        f = (w >> 2 * r) & 3
        if f != 3:
            return (0, 1, -1)[f]
    return 0


def cbd_value(w, eta):
    assert 1 <= eta <= 32
    m = (1 << eta) - 1
    return bin(w & m).count("1") - bin((w >> 32) & m).count("1")


def _cells(n):
    return max(1, n // 8), min(8, n)


def uniform(key, nonce, moduli, n, batch, frame_first=0, prime_first=0, blocks=None):
    """[len(moduli)][batch][n] uint64: slab i under the modulus moduli[i], which is plan prime prime_first + i.  blocks (a list): the blocks every cell
    read are appended, slab by slab"""
    cells, W = _cells(n)
    out = np.zeros((len(moduli), batch, n), dtype=np.uint64)
    for i, q in enumerate(moduli):
        for f in range(batch):
            for c in range(cells):
                words, used = uniform_cell(key, nonce, prime_first + i, frame_first + f, c, int(q), W)
                out[i, f, 8 * c:8 * c + W] = words
                if blocks is not None:
                    blocks.append(used)
    return out


def small_values(key, nonce, kind, n, batch, frame_first=0, eta=None):
    """[batch][n] signed Python integers of the kind "ternary" or "cbd" """
    cells, W = _cells(n)
    k = {"ternary": 0, "cbd": 1}[kind]
    out = np.zeros((batch, n), dtype=np.int64)
    for f in range(batch):
        for c in range(cells):
            cand = candidates(key, nonce, SMALL_TAG, frame_first + f, c, k)[:W]
            out[f, 8 * c:8 * c + W] = [ternary_value(w) if kind == "ternary" else cbd_value(w, eta) for w in cand]
    return out


def small(key, nonce, kind, moduli, n, batch, frame_first=0, eta=None):
    """[len(moduli)][batch][n] uint64: the same small value under every modulus, fully reduced"""
    v = small_values(key, nonce, kind, n, batch, frame_first, eta).astype(object)
    return np.stack([(v % int(q)).astype(np.uint64) for q in moduli])
