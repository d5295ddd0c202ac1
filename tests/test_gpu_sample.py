"""agx_ntt_sample_uniform, _ternary and _cbd on the device, word for word against the Python-integer model (tests/sample_ref.py): n = 2 ... 1024, batches 1, 3
and 5, plans that mix a 2^60 - c prime with the primes next to 2^60 and 2^31 and with 17, ranges that start behind prime 0, frame_first 0, 7 and 2^32 - batch,
eta 1, 21 and 32, both forms (AGX_FORM_NTT against agx_ntt_forward_range of the coefficient form); a batch split over two calls; repeatability and what another
nonce, key or kind changes; odd 8-byte-only placement with guard bands; graph capture; the status rules, rejected calls writing nothing; launches whose
grid-stride loop takes a second step; and BFV end to end on the listings of INTEGRATION.md: s, a, e, u drawn here, a symmetric and a public-key encryption
decrypted by agx_ntt_plain_scale_down."""
import functools

import numpy as np
import pytest

import bfv_conv_ref as bref
import sample_ref as ref
from gpu_util import Layout, arena_for, canary, capture, plan_for_moduli, status_of
from modulus_cases import edge_moduli, prime_below
from rns_ref import oracle_inverse_set

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1
KEY = bytes(range(32))
KEY2 = bytes((7 * i + 3) & 0xFF for i in range(32))
TOP = 1 << 32
TRIP = 2048 * 8 * 256      # work items of one trip round a grid-stride loop (grid_1d, csrc/ntt_kernels.hip)


@functools.lru_cache(maxsize=None)
def _mix(orc, n):
    """a 2^60 - c prime, the primes just above 2^60 and 2^31, the one just below 2^31, and 17 where 2n admits it"""
    e = edge_moduli(orc, n)
    q60c = orc.find_prime(60, n, 0)
    assert 0 < (1 << 60) - q60c < 1 << 28
    return (q60c, e["above60"], e["above31"], e["below31"]) + ((17,) if n <= 8 else ())


def _plan(agx, orc, n, moduli, inverse=False):
    return plan_for_moduli(agx, orc, n, tuple(moduli), inverse)[0]


def _draw(dev, plan, kind, key, nonce, batch, frame_first=0, first=0, count=None, form=COEFF, eta=21):
    """one call into a fresh canary buffer -> the host words, flat [count][batch][n]"""
    count = plan.num_primes - first if count is None else count
    d = dev.to_device(canary(0, count * batch * plan.n))
    _call(plan, kind, key, nonce, d.data_ptr(), batch, frame_first, first, count, form, eta, dev.stream)
    return dev.to_host(d)


def _call(plan, kind, key, nonce, ptr, batch, frame_first, first, count, form, eta, stream):
    if kind == "uniform":
        plan.sample_uniform(key, nonce, ptr, batch, frame_first, first, count, stream)
    elif kind == "ternary":
        plan.sample_ternary(key, nonce, ptr, batch, frame_first, first, count, form, stream)
    else:
        plan.sample_cbd(key, nonce, eta, ptr, batch, frame_first, first, count, form, stream)


def _model(plan, kind, key, nonce, batch, frame_first=0, first=0, count=None, eta=21):
    count = plan.num_primes - first if count is None else count
    moduli = plan.moduli[first:first + count]
    if kind == "uniform":
        return ref.uniform(key, nonce, moduli, plan.n, batch, frame_first, first).reshape(-1)
    return ref.small(key, nonce, kind, moduli, plan.n, batch, frame_first, eta).reshape(-1)


def _first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()


KINDS = (("uniform", None), ("ternary", None), ("cbd", 1), ("cbd", 21), ("cbd", 32))


# ---- word for word against the model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4, 8, 64, 1024])
def test_word_for_word_against_the_model(agx, orc, dev, n):
    """every kind in coefficient form, and the small kinds in NTT form against the plan's forward of those words on the same range"""
    plan = _plan(agx, orc, n, _mix(orc, n))
    P = plan.num_primes
    wide = P - 1 if n < 1024 else 1      # the model walks every cell in Python: fewer slabs at the largest size
    for batch, frame_first, first, count in ((1, 0, 0, P), (3, 7, 1, wide), (5, TOP - 5, 2, min(2, wide)), (3, TOP - 3, P - 1, 1)):
        for kind, eta in KINDS:
            nonce = (1 << 40) + ("uniform", "ternary", "cbd").index(kind)      # the three widths of cbd read the same blocks
            got = _draw(dev, plan, kind, KEY, nonce, batch, frame_first, first, count, COEFF, eta)
            want = _model(plan, kind, KEY, nonce, batch, frame_first, first, count, eta)
            assert np.array_equal(got, want), (n, kind, eta, batch, frame_first, first, count, "first differing words", _first_bad(got, want))
            if kind == "uniform":
                continue
            d = dev.to_device(want)
            plan.forward_range(d.data_ptr(), d.data_ptr(), batch, first, count, dev.stream)
            hat = _draw(dev, plan, kind, KEY, nonce, batch, frame_first, first, count, NTT, eta)
            assert np.array_equal(hat, dev.to_host(d)), (n, kind, eta, batch, "NTT form")
    plan.close()


def test_the_rejection_path_runs_on_the_device(agx, orc, dev):
    """n = 8 under 17, n = 64 under the primes above 2^31 and 2^60: cells that take a third block, as the model counts them; none takes a second under 2^60 - c"""
    for n, name, batch in ((8, "tiny", 64), (64, "above31", 8), (64, "above60", 8), (64, "q60c", 8)):
        q = 17 if name == "tiny" else _mix(orc, n)[("q60c", "above60", "above31").index(name)]
        plan = _plan(agx, orc, n, (q,))
        blocks = []
        want = ref.uniform(KEY, 11, [q], n, batch, blocks=blocks).reshape(-1)
        assert max(blocks) == 1 if name == "q60c" else max(blocks) >= 3, (name, max(blocks))
        got = _draw(dev, plan, "uniform", KEY, 11, batch)
        assert np.array_equal(got, want), (name, _first_bad(got, want))
        plan.close()


# ---- the properties of the definition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,eta", KINDS[:2] + KINDS[3:4])
def test_two_calls_split_at_frame_first_equal_one_call(agx, orc, dev, kind, eta):
    n, batch = 64, 5
    plan = _plan(agx, orc, n, _mix(orc, n))
    for form in (COEFF, NTT):
        for frame_first in (0, 7, TOP - batch):
            whole = _draw(dev, plan, kind, KEY, 3, batch, frame_first, 1, 3, form, eta).reshape(3, batch, n)
            head = _draw(dev, plan, kind, KEY, 3, 2, frame_first, 1, 3, form, eta).reshape(3, 2, n)
            tail = _draw(dev, plan, kind, KEY, 3, 3, frame_first + 2, 1, 3, form, eta).reshape(3, 3, n)
            assert np.array_equal(whole[:, :2], head) and np.array_equal(whole[:, 2:], tail), (kind, form, frame_first)
            # a prime range equals those slabs of the whole plan
            full = _draw(dev, plan, kind, KEY, 3, batch, frame_first, 0, 4, form, eta).reshape(4, batch, n)
            assert np.array_equal(full[1:], whole), (kind, form, frame_first)
    plan.close()


def test_repeatability_and_what_changes_the_words(agx, orc, dev):
    n, batch = 64, 3
    plan = _plan(agx, orc, n, _mix(orc, n))
    for kind, eta in KINDS[:2] + KINDS[3:4]:
        a = _draw(dev, plan, kind, KEY, 9, batch, 0, 0, None, COEFF, eta)
        assert np.array_equal(a, _draw(dev, plan, kind, KEY, 9, batch, 0, 0, None, COEFF, eta)), kind
        for other in (_draw(dev, plan, kind, KEY, 10, batch, eta=eta), _draw(dev, plan, kind, KEY, 9 + (1 << 32), batch, eta=eta), _draw(dev, plan, kind, KEY2, 9, batch, eta=eta),
                      _draw(dev, plan, kind, KEY[:31] + b"\x9f", 9, batch, eta=eta), _draw(dev, plan, kind, KEY, 9, batch, 1, eta=eta)):
            assert np.mean(a != other) > (0.4 if kind == "ternary" else 0.7), kind      # two ternary draws agree on a third of their words
    t, c1, c21 = (_draw(dev, plan, k, KEY, 9, batch, eta=e) for k, e in (("ternary", None), ("cbd", 1), ("cbd", 21)))
    u = _draw(dev, plan, "uniform", KEY, 9, batch)
    assert np.mean(t != c1) > 0.3 and np.mean(c1 != c21) > 0.3 and np.mean(u != t) > 0.9
    plan.close()


# ---- placement -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 64])
@pytest.mark.parametrize("offset", [1, 6])
def test_odd_placement_and_guard_bands(agx, orc, dev, n, offset):
    """d_out at an odd word (8-byte alignment only: the 8-byte stores) and at an even one (the 16-byte stores) of a larger allocation: the model's words, and
    every word outside d_out as it was"""
    batch = 3
    plan = _plan(agx, orc, n, _mix(orc, n))
    for kind, eta in KINDS[:2] + KINDS[3:4]:
        for form in (COEFF,) if kind == "uniform" else (COEFF, NTT):
            lo = Layout(n, 3, batch, offset=offset)
            arena = arena_for(dev, n, (lo, None))
            assert (arena.address(lo.offset) % 16 == 8) == (offset % 2 == 1)
            _call(plan, kind, KEY, 21, arena.address(lo.offset), batch, 7, 1, 3, form, eta, dev.stream)
            img = arena.image()
            assert not arena.faults([(lo, None)], img), (kind, form, "a word outside d_out changed")
            want = _model(plan, kind, KEY, 21, batch, 7, 1, 3, eta)
            if form == NTT:
                d = dev.to_device(want)
                plan.forward_range(d.data_ptr(), d.data_ptr(), batch, 1, 3, dev.stream)
                want = dev.to_host(d)
            assert np.array_equal(arena.frames(lo, img), want), (kind, form, offset)
    plan.close()


@pytest.mark.parametrize("n", [64, 4096])
def test_the_calls_are_graph_capturable(agx, orc, dev, n):
    """the three calls captured on a side stream -- uniform, ternary to NTT form, cbd to coefficient form -- and replayed into zeroed buffers: the eager words"""
    batch = 3
    plan = _plan(agx, orc, n, _mix(orc, n)[:3])
    outs = [dev.empty(3 * batch * n) for _ in range(3)]

    def every(s):
        plan.sample_uniform(KEY, 5, outs[0].data_ptr(), batch, 7, 0, 3, s)
        plan.sample_ternary(KEY, 5, outs[1].data_ptr(), batch, 7, 0, 3, NTT, s)
        plan.sample_cbd(KEY, 5, 21, outs[2].data_ptr(), batch, 7, 1, 2, COEFF, s)

    graph = capture(dev, every, every)
    for _ in range(2):
        for d in outs:
            d.zero_()
        graph.replay()
        dev.sync()
        got = [dev.to_host(d) for d in outs]
        want = [_draw(dev, plan, "uniform", KEY, 5, batch, 7, 0, 3), _draw(dev, plan, "ternary", KEY, 5, batch, 7, 0, 3, NTT), _draw(dev, plan, "cbd", KEY, 5, batch, 7, 1, 2, COEFF, 21)]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2][:2 * batch * n], want[2]), n
        assert not got[2][2 * batch * n:].any()
    if n == 64:
        assert np.array_equal(want[0], _model(plan, "uniform", KEY, 5, batch, 7, 0, 3)) and np.array_equal(want[2], _model(plan, "cbd", KEY, 5, batch, 7, 1, 2, 21))
    plan.close()


def test_status_rules_and_rejected_calls_write_nothing(agx, orc, dev):
    n, batch = 64, 2
    plan = _plan(agx, orc, n, _mix(orc, n))
    P, st = plan.num_primes, dev.stream
    lo = Layout(n, P, batch, offset=0)
    arena = arena_for(dev, n, (lo, canary(100, P * batch * n)))
    before = arena.image()
    out = arena.address(0)
    U, T, C = plan.sample_uniform, plan.sample_ternary, plan.sample_cbd
    calls = {      # (batch, frame_first, prime_first, prime_count) -> the call, key and d_out as given
        "uniform": lambda key, ptr, b, ff, pf, pc, form=COEFF, eta=21: U(key, 1, ptr, b, ff, pf, pc, st),
        "ternary": lambda key, ptr, b, ff, pf, pc, form=COEFF, eta=21: T(key, 1, ptr, b, ff, pf, pc, form, st),
        "cbd": lambda key, ptr, b, ff, pf, pc, form=COEFF, eta=21: C(key, 1, eta, ptr, b, ff, pf, pc, form, st),
    }
    for kind, call in calls.items():
        # NULL key or d_out, in front of every other rule
        for shape in ((batch, 0, 0, P), (batch, 0, P, 1), (batch, TOP, 0, 0), ((1 << 64) - 1, (1 << 64) - 1, 0, P)):
            assert status_of(agx, call, None, out, *shape, 7, 0) == 1 and status_of(agx, call, KEY, 0, *shape, 7, 33) == 1, (kind, shape)
        # a range past P, an empty range
        for pf, pc in ((P, 1), (0, P + 1), (1, P), (0, 0), (0xFFFFFFFF, 2), (2, 0xFFFFFFFF)):
            assert status_of(agx, call, KEY, out, batch, 0, pf, pc) == 5, (kind, pf, pc)
        # frame_first + batch > 2^32
        for b, ff in ((1, TOP), (2, TOP - 1), (batch, (1 << 64) - 1), ((1 << 64) - 1, 2), (0, TOP + 1), (TOP + 1, 0)):
            assert status_of(agx, call, KEY, out, b, ff, 0, P) == 5, (kind, b, ff)
        assert status_of(agx, call, KEY, out + 4, batch, 0, 0, P) == 5      # uint64_t data
        assert status_of(agx, call, KEY, out, 1 << 31, 0, 0, 1) == 5      # a batch past the grid limit
        for ff in (0, 7, TOP):      # an empty batch: nothing launched
            call(KEY, out, 0, ff, 0, P)
    for kind in ("ternary", "cbd"):
        for form in (2, 7, -1):
            assert status_of(agx, calls[kind], KEY, out, batch, 0, 0, P, form) == 5, (kind, form)
    for eta in (0, 33, 64, 0xFFFFFFFF):
        for form in (COEFF, NTT, 7):
            assert status_of(agx, calls["cbd"], KEY, out, batch, 0, 0, P, form, eta) == 5, eta
    dev.sync()
    assert np.array_equal(arena.image(), before), "a rejected call wrote memory"
    # allowed: the last frame numbers, the last prime alone
    calls["cbd"](KEY, out, batch, TOP - batch, P - 1, 1, NTT, 32)
    calls["uniform"](KEY, out, 1, TOP - 1, 0, P)
    dev.sync()
    plan.close()


# ---- launches whose grid-stride loop takes a second step -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,eta", KINDS[:2] + KINDS[3:4])
def test_past_one_grid_stride_trip(agx, orc, dev, kind, eta):
    """n = 1024 (128 cells per frame), 32,771 frames under one 2^60 - c prime: 4,194,688 cells, more than the 4,194,304 threads of one trip.  Judged on the
    device by the range of every word and by two calls split at an odd frame; judged against the model on the first and the last cell, the cells on both sides
    of the trip and a few between"""
    torch = dev.torch
    n, batch, cells = 1024, 32771, 128
    assert batch * cells > TRIP > (batch - 4) * cells
    q = _mix(orc, n)[0]
    plan = _plan(agx, orc, n, (q,))
    frame_first, nonce = TOP - batch - 9, 1 << 63
    d, d2 = dev.empty(batch * n), dev.empty(batch * n)
    d.fill_(-1), d2.fill_(-1)
    _call(plan, kind, KEY2, nonce, d.data_ptr(), batch, frame_first, 0, 1, COEFF, eta, dev.stream)
    head = 16385
    _call(plan, kind, KEY2, nonce, d2.data_ptr(), head, frame_first, 0, 1, COEFF, eta, dev.stream)
    _call(plan, kind, KEY2, nonce, d2.data_ptr() + 8 * head * n, batch - head, frame_first + head, 0, 1, COEFF, eta, dev.stream)
    dev.sync()
    assert torch.equal(d, d2), kind
    if kind == "uniform":
        assert bool(((d >= 0) & (d < q)).all())
        assert float((d >> 59).double().mean()) > 0.45      # the top bit of a 60-bit word: not a buffer of small values
    else:
        bound = 1 if kind == "ternary" else eta
        assert bool(((d <= bound) | (d >= q - bound)).all() & (d >= 0).all() & (d < q).all())
    for e in (0, 1, TRIP - 1, TRIP, TRIP + 1, batch * cells - 1, batch * cells - 2, 12345 * cells + 77):
        f, c = divmod(e, cells)
        got = d[f * n + 8 * c:f * n + 8 * c + 8].cpu().numpy().view(np.uint64)
        if kind == "uniform":
            want = ref.uniform_cell(KEY2, nonce, 0, frame_first + f, c, q, 8)[0]
        else:
            cand = ref.candidates(KEY2, nonce, ref.SMALL_TAG, frame_first + f, c, 0 if kind == "ternary" else 1)
            want = [(ref.ternary_value(w) if kind == "ternary" else ref.cbd_value(w, eta)) % q for w in cand]
        assert got.tolist() == want, (kind, "cell", e)
    plan.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def test_bfv_end_to_end_with_sampled_randomness(agx, orc, dev):
    """The INTEGRATION.md listings "BFV encryption" and "public-key encryption" at n = 64, batch 2, with the parameters of tests/test_gpu_plain.py (BFV_WIDTHS /
    BFV_T, gamma = the first prime of B): s ternary, a uniform, e cbd(21), u ternary, all drawn by the library; two messages per listing decrypt to themselves on
    every coefficient through agx_ntt_plain_scale_down"""
    n, batch = 64, 2
    w = bref.BFV_WIDTHS
    Q = tuple(prime_below(orc, 1 << b, n) for b in w["Q"])
    gamma, t = prime_below(orc, 1 << w["B"][0], n), bref.BFV_T
    L = len(Q)
    plan = _plan(agx, orc, n, Q + (gamma,), inverse=True)
    plain = plan.plain(0, L, L, t)
    slab, st = batch * n, dev.stream
    at = lambda d, words: d.data_ptr() + 8 * words      # noqa: E731
    seed = KEY2      # the caller's 32 bytes; one nonce per draw of a kind
    rng = bref.Rng(2024)
    msgs = [[[rng.below(t) for _ in range(n)] for _ in range(batch)] for _ in range(2)]

    d_shat = dev.empty(L * n)      # the secret: ONE frame per prime, NTT form
    plan.sample_ternary(seed, 0, d_shat.data_ptr(), 1, 0, 0, L, NTT, st)

    def decrypt(d_ct):
        d_phase, d_msg = dev.empty(L * slab), dev.to_device(canary(0, slab))
        d_phase.copy_(d_ct[:L * slab])
        plan.mul_add_galois(d_shat.data_ptr(), at(d_ct, L * slab), d_phase.data_ptr(), batch, 1, 1, True, 0, L, st)      # c_0 + c_1 s
        plain.scale_down(d_phase.data_ptr(), d_msg.data_ptr(), d_phase.data_ptr(), batch, st)
        return dev.to_host(d_msg).reshape(batch, n).tolist()

    def encrypt_symmetric(m, draw):
        """c_1 = a, c_0 = Delta m - a s + e"""
        d_ct, d_m, d_e, d_as = dev.empty(2 * L * slab), dev.to_device(np.array(m, dtype=np.uint64).reshape(-1)), dev.empty(L * slab), dev.empty(L * slab)
        plan.sample_uniform(seed, draw, at(d_ct, L * slab), batch, 0, 0, L, st)
        plan.sample_cbd(seed, draw, 21, d_e.data_ptr(), batch, 0, 0, L, NTT, st)
        plain.scale_up(d_m.data_ptr(), d_ct.data_ptr(), batch, NTT, st)
        plan.mul_add_galois(d_shat.data_ptr(), at(d_ct, L * slab), d_as.data_ptr(), batch, 1, 1, False, 0, L, st)
        plan.sub(d_ct.data_ptr(), d_as.data_ptr(), d_ct.data_ptr(), batch, 0, L, st)
        plan.add(d_ct.data_ptr(), d_e.data_ptr(), d_ct.data_ptr(), batch, 0, L, st)
        return d_ct

    # the public key (p_0, p_1) = (-(a s) + e, a): one frame per prime
    d_pk, d_epk = dev.empty(2 * L * n), dev.empty(L * n)
    plan.sample_uniform(seed, 1000, at(d_pk, L * n), 1, 0, 0, L, st)
    plan.sample_cbd(seed, 1000, 21, d_epk.data_ptr(), 1, 0, 0, L, NTT, st)
    plan.mul_add_galois(d_shat.data_ptr(), at(d_pk, L * n), d_pk.data_ptr(), 1, 1, 1, False, 0, L, st)
    plan.negate(d_pk.data_ptr(), d_pk.data_ptr(), 1, 0, L, st)
    plan.add(d_pk.data_ptr(), d_epk.data_ptr(), d_pk.data_ptr(), 1, 0, L, st)

    def encrypt_public(m, draw):
        """c_0 = p_0 u + e_1 + Delta m, c_1 = p_1 u + e_2"""
        d_ct, d_m, d_u, d_e = dev.empty(2 * L * slab), dev.to_device(np.array(m, dtype=np.uint64).reshape(-1)), dev.empty(L * slab), dev.empty(2 * L * slab)
        plan.sample_ternary(seed, draw, d_u.data_ptr(), batch, 0, 0, L, NTT, st)
        plan.sample_cbd(seed, 100 + 2 * draw, 21, d_e.data_ptr(), batch, 0, 0, L, NTT, st)
        plan.sample_cbd(seed, 101 + 2 * draw, 21, at(d_e, L * slab), batch, 0, 0, L, NTT, st)
        plan.mul_add_galois(d_pk.data_ptr(), d_u.data_ptr(), d_ct.data_ptr(), batch, 1, 1, False, 0, L, st)
        plan.mul_add_galois(at(d_pk, L * n), d_u.data_ptr(), at(d_ct, L * slab), batch, 1, 1, False, 0, L, st)
        plan.add(d_ct.data_ptr(), d_e.data_ptr(), d_ct.data_ptr(), batch, 0, L, st)
        plan.add(at(d_ct, L * slab), at(d_e, L * slab), at(d_ct, L * slab), batch, 0, L, st)
        plain.scale_up(d_m.data_ptr(), d_e.data_ptr(), batch, NTT, st)      # Delta m, in the place of e_1
        plan.add(d_ct.data_ptr(), d_e.data_ptr(), d_ct.data_ptr(), batch, 0, L, st)
        return d_ct

    for o in range(2):
        assert decrypt(encrypt_symmetric(msgs[o], 1 + o)) == msgs[o], ("symmetric", o)
        assert decrypt(encrypt_public(msgs[o], 1 + o)) == msgs[o], ("public key", o)
    # what was drawn is what the model draws: the secret is ternary, and two encryptions of one message differ
    s = oracle_inverse_set(orc, n, Q, dev.to_host(d_shat).reshape(L, n))
    assert np.array_equal(s.reshape(-1), ref.small(seed, 0, "ternary", Q, n, 1).reshape(-1))
    a, b = dev.to_host(encrypt_public(msgs[0], 7)), dev.to_host(encrypt_public(msgs[0], 8))
    assert np.mean(a != b) > 0.99
    plain.close()
    plan.close()
