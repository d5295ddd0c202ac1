"""What tests/test_q60c_skip_model.py (CPU) and tests/test_gpu_fwd_q60c_skip.py share: the moduli on both sides of the class limit of the skip form
of the two-twiddle butterfly (csrc/modarith.hpp: ct_butterfly_q60c_fold forms 2 / 3, q60c_skip_bounds; csrc/ntt_kernels.hpp: kQ60cSkipMaxC), and an
integer model of the whole n = 4096 forward transform in that schedule, in Python integers, which checks every intermediate word against [0, 2^64).

The model follows the kernel operation for operation: q = 2^60 - c; a table slot holds w and wC = w 2^32 mod q, each split at bit 29; on the even
stages x is first reduced by its top four bits, r = (x mod 2^60) + (x >> 60) c; then
    hi = y0 wh + y1 wCh,   x' = tx + y0 wl + y1 wCl + hl 2^29 + hh 2c  (one chain, in this order),   y' = 2 tx + 7q - x'  (mod 2^64) = tx + 7q - Q.
The transform is the oracle's: radix-2 Cooley-Tukey, natural order in, bit-reversed out, twiddle index m + i."""
M64 = 1 << 64
W32 = (1 << 32) - 1
N = 4096
LOG_N = 12
TWO_N = 2 * N
SKIP_MAX_C = 1 << 27      # kQ60cSkipMaxC: the class the library's host code tests and q60c_skip_bounds proves (the bounds hold up to 2^27 + 1)


class WordOverflow(AssertionError):
    """a word of the model left [0, 2^64)"""


def _word(v, what):
    if not 0 <= v < M64:
        raise WordOverflow(f"{what} = {v} is outside [0, 2^64)")
    return v


def prime_at_or_below_c(orc, c_top):
    """q = 2^60 - c, the prime = 1 (mod 2n) with the largest c <= c_top; returns (q, c)"""
    c = c_top - ((c_top + 1) % TWO_N)      # c = -1 (mod 2n)
    while not orc.is_prime((1 << 60) - c):
        c -= TWO_N
    assert c > 0
    return (1 << 60) - c, c


def prime_above_c(orc, c_floor):
    """... with the smallest c > c_floor"""
    c = c_floor + 1
    c += (-(c + 1)) % TWO_N
    while not orc.is_prime((1 << 60) - c):
        c += TWO_N
    assert c > c_floor and c < (1 << 28)
    return (1 << 60) - c, c


def fold_slot(w, q):
    """(wl, wh, wCl, wCh): what the pass table holds for the twiddle w (agx::fold_twiddle_pack)"""
    wc = (w << 32) % q
    return w & ((1 << 29) - 1), w >> 29, wc & ((1 << 29) - 1), wc >> 29


def reduce_top4(x, c):
    return (x & ((1 << 60) - 1)) + (x >> 60) * c


def butterfly(tx, y, slot, q, c, hi_words=None):
    """one butterfly on the (already reduced, or passed through) x word tx; every word checked.  hi_words: (hl, hh) in place of the words of hi --
    the worst-case butterfly feeds each word its own maximum, as the static proof does"""
    wl, wh, wcl, wch = slot
    y0, y1 = y & W32, y >> 32
    hi = _word(y0 * wh + y1 * wch, "hi")
    hl, hh = hi_words if hi_words else (hi & W32, hi >> 32)
    s = _word(tx + y0 * wl, "tx + y0 wl")
    s = _word(s + y1 * wcl, "... + y1 wCl")
    s = _word(s + (hl << 29), "... + hl 2^29")
    xn = _word(s + hh * 2 * c, "x'")
    yn = _word(tx + 7 * q - (xn - tx), "y' = tx + 7q - Q")
    assert (2 * tx + 7 * q - xn) % M64 == yn      # what the kernel computes, 2 tx possibly wrapped
    return xn, yn


def forward_model(x, q, tw, reduces=lambda s: s % 2 == 0):
    """the transform of one frame x (any 64-bit words) in Python integers; returns the fully reduced outputs"""
    c = (1 << 60) - q
    x = [int(v) for v in x]
    slots = [fold_slot(int(w), q) for w in tw]
    m, t = 1, N // 2
    for stage in range(LOG_N):
        red = reduces(stage)
        for i in range(m):
            slot, j0 = slots[m + i], 2 * i * t
            for j in range(j0, j0 + t):
                tx = reduce_top4(x[j], c) if red else x[j]
                x[j], x[j + t] = butterfly(tx, x[j + t], slot, q, c)
        m, t = 2 * m, t // 2
    out = []
    for v in x:      # reduce_final_q60c
        r = reduce_top4(v, c)
        assert r < 2 * q
        out.append(r - q if r >= q else r)
    return out


def worst_case_pair(q):
    """a reducing butterfly and the unreduced one behind it with every operand word at its own maximum (what q60c_skip_bounds bounds): x any word,
    y words 2^32 - 1, the low halves 2^29 - 1, the high halves those of q - 1, both words of hi 2^32 - 1.  Raises WordOverflow where a word leaves
    [0, 2^64); returns the largest output otherwise"""
    c = (1 << 60) - q
    slot = ((1 << 29) - 1, (q - 1) >> 29, (1 << 29) - 1, (q - 1) >> 29)
    worst = lambda tx: butterfly(tx, M64 - 1, slot, q, c, hi_words=(W32, W32))[0]      # noqa: E731
    worst(0)      # the smallest x: y' = 7q - Q must not go negative (what limits c)
    x1 = worst(reduce_top4(M64 - 1, c))      # the largest reduced x: x' must not wrap
    # an output of the reducing stage is at most tx + 7q (x' when Q is 7q, y' when Q is 0); the stage behind it takes that word as it comes
    tx2 = _word(reduce_top4(M64 - 1, c) + 7 * q, "tx + 7q")
    x2 = worst(tx2)
    return max(x1, x2, _word(tx2 + 7 * q, "tx + 7q behind a reducing stage"))
