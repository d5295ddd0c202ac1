"""The case builders and runners that more than one GPU test file of the RNS calls uses: the key switch's shapes, cases and one-call runner
(test_gpu_keyswitch.py, test_gpu_keyswitch_hoisted.py, test_hoist_reference.py) and the inner product's operands, layouts and device words
(test_gpu_inner_product.py, test_gpu_inner_product_galois.py).  The expected words come from rns_ref.py.  Cases are computed once and read-only."""
import functools

import numpy as np

from gpu_util import Layout, canary
from rns_ref import active_of, digits_of, keyswitch_ref, spread

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
