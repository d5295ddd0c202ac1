"""The case builders and runners that more than one GPU test file of the RNS calls uses: the key switch's shapes, cases and one-call runner
(test_gpu_keyswitch.py, test_gpu_keyswitch_hoisted.py, test_hoist_reference.py) and the inner product's operands, layouts and device words
(test_gpu_inner_product.py, test_gpu_inner_product_galois.py), the key switch's wide shapes (test_gpu_keyswitch_wide.py, test_hoist_reference.py) and the
bases and cases of the sweep over every source count (test_gpu_source_counts.py, test_rns_ref.py).  The expected words come from rns_ref.py and
moddown_modes_ref.py.  Cases are computed once and read-only."""
import functools

import numpy as np

from gpu_util import Layout, canary
from moddown_modes_ref import mod_down_mode, special_sources
from rns_ref import active_of, convert, digits_of, keyswitch_ref, oracle_forward_set, residues, special_values, spread

# ---- the key switch: (q_count, p_first, p_count, alpha) on a plan of six primes ----------------------------------------------------------------
TOP, LOWER, FOUR_DIGITS, ONE_DIGIT = (4, 4, 2, 2), (3, 4, 2, 2), (4, 5, 1, 1), (4, 4, 2, 4)
SHAPES = (TOP, LOWER, FOUR_DIGITS, ONE_DIGIT)
SHAPE_IDS = ["top", "lower", "four-digits", "one-digit"]
FIVE = SHAPES + ((3, 3, 3, 2),)
FIVE_IDS = SHAPE_IDS + ["three-special"]


@functools.lru_cache(maxsize=None)
def keyswitch_case(orc, n, moduli, shape, batch, seed):
    """(chat, key reduced; chat, key spread over [0,4q); the expected words), all flat, computed once per case (read-only).  Any residues are
    NTT-form frames; the first frame opens with words 0 and q - 1"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    D = len(digits_of(shape))
    rng = np.random.default_rng(seed)
    chat = np.stack([rng.integers(0, int(q), size=(batch, n), dtype=np.uint64) for q in active[:q_count]])
    chat[:, 0, 0] = 0
    chat[:, 0, 1] = np.array(active[:q_count], dtype=np.uint64) - np.uint64(1)
    key = np.stack([rng.integers(0, int(q), size=(D, 2, n), dtype=np.uint64) for q in active], axis=2)      # [D][2][A][n]
    want = keyswitch_ref(orc, n, moduli, shape, chat, key, batch)
    lkey = np.moveaxis(spread(rng, np.moveaxis(key, 2, 0), active), 0, 2)      # drawn with the prime on axis 0
    out = (chat.reshape(-1), key.reshape(-1), spread(rng, chat, active[:q_count]).reshape(-1), np.ascontiguousarray(lkey).reshape(-1), want.reshape(-1))
    for w in out:
        w.setflags(write=False)
    return out


def run_keyswitch(dev, ks, chat, key, batch):
    """agx_ntt_keyswitch_apply into a canary-filled out with a scratch of exactly the reported size; returns the output words and checks chat and
    key unchanged"""
    d_chat, d_key = dev.to_device(chat), dev.to_device(key)
    d_out, d_s = dev.to_device(canary(0, 2 * chat.size)), dev.empty(ks.scratch_words(batch))
    ks.apply(d_chat.data_ptr(), d_key.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), batch, dev.stream)
    got = dev.to_host(d_out)
    assert np.array_equal(dev.to_host(d_chat), chat) and np.array_equal(dev.to_host(d_key), key), "an input changed"
    return got


# ---- the key switch at wide shapes, on a plan of 33 primes (test_gpu_keyswitch_wide.py, test_hoist_reference.py) ---------------------------------
WIDE_PRIMES = 33
TWO_FULL_DIGITS = (12, 12, 6, 6)      # two full digits, six sources both ways
WIDE = (TWO_FULL_DIGITS,
        (13, 14, 7, 5),               # special primes apart (two ModUp bases per digit), a short last digit of 3
        (16, 16, 1, 1),               # sixteen digits, the limit: a 16-term inner product
        (24, 24, 8, 8),               # A = 32
        (16, 16, 16, 16),             # alpha and p_count at their limits, one digit
        (9, 20, 9, 9))                # capacity 16 partly filled, far-apart special primes
WIDE_IDS = ["two-full-digits", "apart-short-last", "sixteen-digits", "thirty-two-active", "limits-one-digit", "nine-far-apart"]


# ---- every source count: bases on a plan of 19 primes (test_gpu_source_counts.py, test_rns_ref.py) -------------------------------------------------
SWEEP_PRIMES = 19
SOURCE_COUNTS = tuple(range(1, 17))
MIXED_WIDTHS = tuple([30, 60, 61, 62][k % 4] for k in range(SWEEP_PRIMES))


def extend_shape(S):
    """(source first, source count, target first, target count): sources [0, S), targets [S - 1, S + 2) -- the first target is the last source, the
    other two are foreign"""
    return 0, S, S - 1, 3


def mod_down_shape(S):
    """targets [0, 3), sources [3, 3 + S)"""
    return 3, S, 0, 3


@functools.lru_cache(maxsize=None)
def extend_sweep_case(orc, n, moduli, S, batch, seed):
    """agx_ntt_basis_extend on extend_shape(S): (x reduced, x spread over [0,4q), {0: the coefficient-form words, 1: their NTT form}), flat, computed
    once per case (read-only).  Frame 0 opens with rns_ref.special_values (8 + S of them), random behind; the first target's words are x_{S-1}"""
    sf, S, df, T = extend_shape(S)
    src, dst = moduli[sf:sf + S], moduli[df:df + T]
    rng = np.random.default_rng(seed)
    x = np.stack([rng.integers(0, int(q), size=(batch, n), dtype=np.uint64) for q in src])
    special = residues(special_values(src), src)
    assert special.shape[1] == 8 + S <= n
    x[:, 0, :special.shape[1]] = special
    coeff = convert(x, src, dst)
    assert np.array_equal(coeff[0], x[S - 1].reshape(-1)), "a target that is a source must get its residue back"
    out = (x.reshape(-1), spread(rng, x, src).reshape(-1), {0: coeff.reshape(-1), 1: oracle_forward_set(orc, n, dst, coeff).reshape(-1)})
    for w in (*out[:2], *out[2].values()):
        w.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mod_down_sweep_case(orc, n, moduli, S, batch, seed, t, mode):
    """agx_ntt_basis_mod_down_mode on mod_down_shape(S): (xq, xp reduced; xq, xp spread over [0,4q); the expected words [3][batch][n]), NTT form, flat,
    computed once per case (read-only).  The sources' coefficient form opens frame 0 with moddown_modes_ref.special_sources(src, t, mode)"""
    sf, S, df, T = mod_down_shape(S)
    src, dst = moduli[sf:sf + S], moduli[df:df + T]
    rng = np.random.default_rng(seed)
    a = np.stack([rng.integers(0, int(q), size=(batch, n), dtype=np.uint64) for q in dst])
    p = np.stack([rng.integers(0, int(q), size=(batch, n), dtype=np.uint64) for q in src])
    special = special_sources(src, t, mode)
    p[:, 0, :special.shape[1]] = special
    xq, xp = oracle_forward_set(orc, n, dst, a), oracle_forward_set(orc, n, src, p)
    want = oracle_forward_set(orc, n, dst, mod_down_mode(a, p, src, dst, t, mode))
    out = (xq.reshape(-1), xp.reshape(-1), spread(rng, xq, dst).reshape(-1), spread(rng, xp, src).reshape(-1), want.reshape(-1))
    for w in out:
        w.setflags(write=False)
    return out


# ---- the inner product ------------------------------------------------------------------------------------------------------------------------
# work items one grid-stride trip of the launcher covers: at most 2048 * 8 workgroups of 256 threads (grid_1d, csrc/ntt_kernels.hip), one item a
# 16-byte pair of words when all three bases are 16-byte aligned and one word otherwise
TRIP = 2048 * 8 * 256


@functools.lru_cache(maxsize=None)
def inner_operands(n, moduli, batch, seed):
    """(a [16][P][batch][n], b [16][2][P][batch][n]) reduced, and the same spread over [0, 4q): drawn once per shape, every case takes its leading
    terms and outputs (read-only)"""
    rng = np.random.default_rng(seed)
    P = len(moduli)
    a = np.stack([rng.integers(0, q, size=(16, batch, n), dtype=np.uint64) for q in moduli], axis=1)
    b = np.stack([rng.integers(0, q, size=(16, 2, batch, n), dtype=np.uint64) for q in moduli], axis=2)
    a[0, :, 0, :2] = 0      # a zero word and the largest one in every prime's first frame
    a[0, :, 0, 2:4] = b[0, 0, :, 0, 2:4] = (np.array(moduli, dtype=np.uint64) - np.uint64(1))[:, None]
    assert a.shape == (16, P, batch, n) and b.shape == (16, 2, P, batch, n)
    out = (a, b, spread(rng, a, moduli, 1), spread(rng, b, moduli, 2))
    for w in out:
        w.setflags(write=False)
    return out


def inner_layouts(n, P, batch, terms, outputs, bb, offsets):
    """a, bhat and c as frame sets of terms P, terms outputs P and outputs P `primes`, placed one behind the other at the given parities"""
    la = Layout(n, terms * P, batch, offset=offsets[0])
    lb = Layout(n, terms * outputs * P, bb, offset=la.span() + 6 + (la.span() + 6 + offsets[1]) % 2)
    lc = Layout(n, outputs * P, batch, offset=lb.span() + 10 + (lb.span() + 10 + offsets[2]) % 2)
    assert [l.offset % 2 for l in (la, lb, lc)] == [o % 2 for o in offsets]
    return la, lb, lc


def device_words(torch, dev, count, q, seed):
    """`count` words uniform in [0, 4q) on the device"""
    g = torch.Generator(device=dev.device)
    g.manual_seed(seed)
    return torch.randint(0, 4 * int(q), (count,), generator=g, device=dev.device, dtype=torch.int64)
