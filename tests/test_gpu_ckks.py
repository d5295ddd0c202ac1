"""agx_ntt_ckks_encode and agx_ntt_ckks_decode on the device.  Word for word against the float64 model (tests/ckks_ref.py), doubles compared by bit pattern:
every size from 2 to 32768 with full, eighth and single slots, both sides of the step from the LDS planes (8192 slots) to the global route (16384), 60-bit
primes of the class 2^60 - c and a plan that mixes a 31-bit, the smallest, a 62-bit and a 60-bit prime behind q_first = 1, count below q_count, the scales
2^30, 2^40 and 2^100 (the last: residues of doubles past 2^63), slots 0, +-1 and +-2^20, one frame of NaN and +-Inf.  AGX_FORM_NTT against the plan's range
transforms; a batch against its frames one by one; the two accuracy bounds of the definition on the device's own output against exact_*; rotation,
conjugation and the product through agx_ntt_automorphism and agx_ntt_polymul_ntt; the statuses in their order with nothing written; graph capture.
One encrypted run at n = 64 on the INTEGRATION.md listing: sampled a and e, symmetric encryption, multiply-plain, agx_ntt_rescale, one hoisted rotation,
decryption and decode at Delta^2 / q_last on a prefix of the handle.  "The plan's device not current" needs a second GPU: with one device visible that rule
cannot be broken, and its test says so and checks nothing."""
import functools
import math

import numpy as np
import pytest

import ckks_ref as ref
from gpu_util import canary, capture, moduli_for, plan_for_moduli, status_of
from modulus_cases import edge_moduli
from rns_ref import oracle_forward_set, oracle_inverse_set, rotation_bound, rotation_key_case

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1
U = 2.0 ** -53


class Doubles:
    """device arrays of doubles beside the DeviceHelper's words"""

    def __init__(self, dev):
        self.dev, self.torch = dev, dev.torch

    def put(self, z):
        z = np.ascontiguousarray(z, dtype=np.complex128)
        return self.torch.from_numpy(z.view(np.float64).copy()).to(self.dev.device)

    def filled(self, count, value=-7.25):
        return self.torch.full((int(count),), value, dtype=self.torch.float64, device=self.dev.device)

    def get(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _moduli(agx, orc, n, kind):
    if kind == "q60":
        return tuple(agx.find_primes(60, n, 3))
    e = edge_moduli(orc, n)
    return (e["below60"], e["below31"], e["min"], e["below62"], e["below40"])      # the handle starts at prime 1: 31-bit, the smallest, the 62-bit edge, 40-bit


@functools.lru_cache(maxsize=None)
def _slots(s, batch, seed, special):
    """[batch][s] slots with |z_j| <= 1; special: 0, +-1, +-2^20 in frame 0 and NaN, +-Inf in frame 1 (the other frames stay finite)"""
    rng = np.random.default_rng(seed)
    z = (rng.uniform(-1, 1, (batch, s)) + 1j * rng.uniform(-1, 1, (batch, s))) / math.sqrt(2)
    if special:
        fixed = [0, 1, -1, 2.0 ** 20, -(2.0 ** 20), 1j, -2.0 ** 20 * 1j, 0.5 - 0.5j]
        z[0, :min(s, len(fixed))] = fixed[:s]
        if batch > 1:
            z[1, :min(s, 3)] = [complex(math.nan, 1), complex(math.inf, 0), complex(0, -math.inf)][:s]
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _residues(Q, batch, n, seed):
    """[L][batch][n] fully reduced words: uniform, with the edges of the centred range (0, +-1, +-(D - 1) / 2 and their neighbours) in front of frame 0"""
    rng = np.random.default_rng(seed)
    x = np.array([rng.integers(0, q, size=(batch, n), dtype=np.uint64) for q in Q])
    D = math.prod(Q)
    for k, X in enumerate([0, 1, -1, (D - 1) // 2, -((D - 1) // 2), (D - 1) // 2 - 1, -((D - 1) // 2) + 1, Q[0], -Q[0]][:n]):
        for i, q in enumerate(Q):
            x[i, 0, k] = X % q
    x.setflags(write=False)
    return x


def _run_encode(agx, dev, ck, z, n, L, scale, form=COEFF):
    dd = Doubles(dev)
    batch, s = z.shape
    d_z, d_out = dd.put(z), dev.to_device(canary(0, L * batch * n))
    ck.encode(d_z.data_ptr(), s, scale, d_out.data_ptr(), batch, L, form, dev.stream)
    got = dev.to_host(d_out).reshape(L, batch, n)
    assert np.array_equal(_bits(dd.get(d_z).reshape(-1)), _bits(z.view(np.float64).reshape(-1))), "d_z changed"
    return got


def _run_decode(agx, dev, ck, x, n, L, scale, s, form=COEFF, scratch="apart"):
    dd = Doubles(dev)
    batch = x.shape[1]
    d_x, d_z = dev.to_device(x.reshape(-1)), dd.filled(2 * batch * s)
    d_s = None if scratch is None else d_x if scratch == "same" else dev.to_device(canary(3, L * batch * n))
    ck.decode(d_x.data_ptr(), form, L, scale, d_z.data_ptr(), s, None if d_s is None else d_s.data_ptr(), batch, dev.stream)
    got = dd.get(d_z).view(np.complex128).reshape(batch, s)
    if scratch != "same":
        assert np.array_equal(dev.to_host(d_x), x.reshape(-1)), "d_x changed"
    return got


def _same_doubles(got, want, what):
    g, w = _bits(got.view(np.float64).reshape(-1)), _bits(want.view(np.float64).reshape(-1))
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, "first differing doubles", bad[:4].tolist(), got.reshape(-1).view(np.float64)[bad[:4]].tolist(), want.reshape(-1).view(np.float64)[bad[:4]].tolist())


def _same_words(got, want, what):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (what, "first differing words", bad[:4].tolist(), got.reshape(-1)[bad[:4]].tolist(), want.reshape(-1)[bad[:4]].tolist())


SIZES = (2, 8, 64, 1024, 4096, 16384, 32768)
SCALES = (2.0 ** 30, 2.0 ** 40, 2.0 ** 100)


def _cases():
    out = []
    for i, n in enumerate(SIZES):
        slots = sorted({n // 2, max(1, n // 8), 1} | ({8192} if n == 32768 else set()))      # n = 32768: 16384 slots go the global route, 8192 the last LDS one
        for k, s in enumerate(slots):
            out.append((n, s, "q60", SCALES[(i + k) % 3], 3))
    out += [(8, 4, "mixed", SCALES[0], 3), (8, 1, "mixed", SCALES[2], 3), (64, 32, "mixed", SCALES[1], 3), (64, 4, "mixed", SCALES[2], 3),
            (4096, 2048, "mixed", SCALES[2], 3), (4096, 512, "mixed", SCALES[0], 3), (64, 32, "q60", SCALES[2], 67), (32768, 16384, "q60", SCALES[2], 3),
            (4096, 2048, "q60", SCALES[2], 3), (2, 1, "q60", SCALES[2], 3)]
    return out


@pytest.mark.parametrize("n,s,kind,scale,batch", _cases(), ids=lambda v: str(int(math.log2(v))) + "b" if isinstance(v, float) else str(v))
def test_word_for_word_against_the_model(agx, orc, dev, n, s, kind, scale, batch):
    moduli = _moduli(agx, orc, n, kind)
    plan = agx.Plan(n, list(moduli))
    q_first, q_count = (0, 3) if kind == "q60" else (1, 4)
    ck = plan.ckks(q_first, q_count)
    assert ck.info()[:3] == (q_first, q_count, n // 2)
    z = _slots(s, batch, 100 + n + s, True)
    # every prefix serves (a level drops primes from the end); the large sizes take one prefix below q_count, the global route (16384 slots) all three
    for L in sorted({q_count, q_count - 1, 1}) if n <= 4096 or s == 16384 else (q_count - 1,):
        Q = moduli[q_first:q_first + L]
        _same_words(_run_encode(agx, dev, ck, z, n, L, scale), ref.encode(z, n, Q, scale), ("encode", n, s, kind, L))
        x = _residues(Q, batch, n, 7 + n)
        _same_doubles(_run_decode(agx, dev, ck, x, n, L, scale, s, scratch=None), ref.decode(x, n, Q, scale, s), ("decode", n, s, kind, L))
    if batch > 1:      # the frame of NaN and infinities: every slot reaches every coefficient from two slots on, so all are 0; a single slot (NaN, 1) zeroes
        got = _run_encode(agx, dev, ck, z, n, 1, scale)      # its real coefficient only; the neighbouring frames are judged above
        assert not got[:, 1].any() if s > 1 else got[0, 1, 0] == 0 and got[0, 1, n // 2] == round(scale) % moduli[q_first]
        assert got[:, 2].any()
    ck.close()
    plan.close()


@pytest.mark.parametrize("n,s", [(64, 32), (64, 4), (4096, 2048), (32768, 16384)])
def test_forms_and_batches_agree(agx, orc, dev, n, s):
    """AGX_FORM_NTT encode = agx_ntt_forward_range of the coefficient form; NTT-form decode = coefficient-form decode of agx_ntt_inverse_range, for reduced
    and lazy words, the scratch apart and the scratch the operand; a batch in one call = its frames one by one"""
    moduli = tuple(agx.find_primes(60, n, 4))
    plan = agx.Plan(n, list(moduli))
    ck, batch, L, scale = plan.ckks(1, 3), 3, 2, 2.0 ** 40
    Q = moduli[1:1 + L]
    z = _slots(s, batch, 5, False)
    coeff = _run_encode(agx, dev, ck, z, n, L, scale, COEFF)
    d = dev.to_device(coeff.reshape(-1))
    plan.forward_range(d.data_ptr(), d.data_ptr(), batch, 1, L, dev.stream)
    xhat = dev.to_host(d)
    _same_words(_run_encode(agx, dev, ck, z, n, L, scale, NTT), xhat, ("ntt encode", n, s))
    for f in range(batch):
        _same_words(_run_encode(agx, dev, ck, z[f:f + 1], n, L, scale, COEFF), coeff[:, f:f + 1], ("frame", f))
    want = _run_decode(agx, dev, ck, coeff, n, L, scale, s, COEFF, None)
    rng = np.random.default_rng(9)
    lazy = xhat.reshape(L, -1) + np.array([rng.integers(0, 4, size=batch * n, dtype=np.uint64) * np.uint64(q) for q in Q])
    for words in (xhat, lazy):
        for scratch in ("apart", "same"):
            _same_doubles(_run_decode(agx, dev, ck, words.reshape(L, batch, n), n, L, scale, s, NTT, scratch), want, ("ntt decode", n, s, scratch))
    assert ck.info()[3] >= 2 and ck.info()[4] >= 2
    ck.close()
    plan.close()


def _decode_bound(X, s, L, scale):
    t = math.log2(2 * s)
    return (8 * t + 4 * L + 2) * U * math.sqrt(s) * math.sqrt(sum(float(v) ** 2 for v in X)) / scale


def _encode_slack(z, s, scale):
    t = math.log2(2 * s)
    return (8 * t + 2) * U * scale * float(np.linalg.norm(z)) / math.sqrt(s)


@pytest.mark.parametrize("n,scale", [(64, 2.0 ** 40), (4096, 2.0 ** 30), (32768, 2.0 ** 30)])
def test_accuracy_of_the_device_output(agx, orc, dev, n, scale):
    """the two bounds of the definition, on sampled indices, against the closed forms in high precision:
    decode |z_j - exact| <= (8t + 4l + 2) u sqrt(s) |X| / Delta;  encode |c_k - Delta w_k| <= 1/2 + E, E = (8t + 2) u Delta |z| / sqrt(s), and c_k the
    nearest integer wherever Delta w_k is farther than E from a half-integer"""
    s, L = n // 2, 2
    moduli = tuple(agx.find_primes(60, n, L))
    plan = agx.Plan(n, list(moduli))
    ck = plan.ckks(0, L)
    z = _slots(s, 1, 11, False)
    c = _run_encode(agx, dev, ck, z, n, L, scale)
    X = ref.centred([c[i][0].tolist() for i in range(L)], moduli)
    ks = sorted({0, 1, s // 2, s - 1, 5 % s, (s // 3) | 1})
    E = _encode_slack(z[0], s, scale)
    exact = ref.exact_encode(z[0], s, ks)
    classed = 0
    for k in ks:
        for idx, part in ((k, exact[k].real), (k + s, exact[k].imag)):
            target = ref.scaled(scale, part)
            err = ref.distance(X[idx], target)
            print("encode", n, idx, "error", err, "bound", 0.5 + E)
            assert err <= 0.5 + E, (n, idx, err, E)
            nearest, margin = ref.nearest_and_margin(target)
            if margin > E:
                classed += 1
                assert X[idx] == nearest, (n, idx, X[idx], nearest)
    assert classed >= 2 * len(ks) - 1      # the class holds at least 99 % of the coefficients (tests/test_ckks_reference.py): at most one sample outside
    got = _run_decode(agx, dev, ck, c, n, L, scale, s, COEFF, None)
    bound = _decode_bound(X, s, L, scale)
    zz = ref.exact_decode(X, n, s, scale, ks)
    for j in ks:
        err = max(ref.distance(got[0][j].real, zz[j].real), ref.distance(got[0][j].imag, zz[j].imag))
        print("decode", n, j, "error", err, "bound", bound)
        assert err <= bound, (n, j, err, bound)
    ck.close()
    plan.close()


@pytest.mark.parametrize("n", [64, 4096])
def test_rotation_conjugation_and_product_through_the_existing_calls(agx, orc, dev, n):
    """decode(automorphism(encode z, 5^r)) = z rotated left by r, g = 2n - 1 conjugates, decode(polymul(encode z, encode z'), Delta^2) = z o z': within the decode
    bound plus the encode rounding carried to the slots, (2s)(1/2 + E) / Delta per encoded operand (a product carries each operand's, times the other's
    largest slot, and their product)"""
    s, L, scale = n // 2, 2, 2.0 ** 40
    moduli = tuple(agx.find_primes(60, n, L))
    plan = agx.Plan(n, list(moduli))
    ck, dd = plan.ckks(0, L), Doubles(dev)
    z, z2 = _slots(s, 1, 21, False), _slots(s, 1, 22, False)
    words = L * n
    d_a, d_b = dev.empty(words), dev.empty(words)
    rounding = (2 * s) * (0.5 + _encode_slack(z[0], s, scale)) / scale
    ck.encode(dd.put(z).data_ptr(), s, scale, d_a.data_ptr(), 1, L, COEFF, dev.stream)
    for g, want in ((agx.galois_element(n, 1), np.roll(z[0], -1)), (agx.galois_element(n, 5), np.roll(z[0], -5)), (2 * n - 1, np.conj(z[0]))):
        plan.automorphism(d_a.data_ptr(), d_b.data_ptr(), 1, g, COEFF, dev.stream)
        x = dev.to_host(d_b).reshape(L, 1, n)
        got = _run_decode(agx, dev, ck, x, n, L, scale, s, COEFF, None)[0]
        tol = _decode_bound(ref.centred([x[i][0].tolist() for i in range(L)], moduli), s, L, scale) + rounding
        err = float(np.abs(got - want).max())
        print("galois", n, g, "error", err, "tolerance", tol)
        assert err <= tol, (g, err, tol)
    d_bhat, d_c = dev.empty(words), dev.empty(words)
    ck.encode(dd.put(z2).data_ptr(), s, scale, d_bhat.data_ptr(), 1, L, NTT, dev.stream)
    plan.polymul_ntt(d_a.data_ptr(), d_bhat.data_ptr(), d_c.data_ptr(), 1, None, dev.stream)
    x = dev.to_host(d_c).reshape(L, 1, n)
    got = _run_decode(agx, dev, ck, x, n, L, scale * scale, s, COEFF, None)[0]
    e1, e2 = rounding, (2 * s) * (0.5 + _encode_slack(z2[0], s, scale)) / scale
    tol = _decode_bound(ref.centred([x[i][0].tolist() for i in range(L)], moduli), s, L, scale * scale) + e1 * float(np.abs(z2).max()) + e2 * float(np.abs(z).max()) + e1 * e2
    err = float(np.abs(got - z[0] * z2[0]).max())
    print("product", n, "error", err, "tolerance", tol)
    assert err <= tol, (err, tol)
    ck.close()
    plan.close()


def test_statuses_in_their_order_and_nothing_written(agx, orc, dev):
    n, batch, s, scale = 64, 2, 8, 2.0 ** 30
    a, b, c = agx.find_primes(60, n, 3)
    plan = agx.Plan(n, [a, b, c])
    C = lambda p, first, count: agx.Ckks(p, first, count).close()      # noqa: E731
    for first, count in ((0, 0), (0, 4), (3, 1), (2, 2), (0, 17), (0xffffffff, 2)):
        assert status_of(agx, C, plan, first, count) == 5, (first, count)
    twice = plan_for_moduli(agx, orc, n, (a, b, a), inverse=False)[0]
    assert status_of(agx, C, twice, 0, 3) == 3 and status_of(agx, C, twice, 0, 2) == 0 and status_of(agx, C, twice, 1, 2) == 0
    ck, dd = plan.ckks(0, 3), Doubles(dev)
    words = 3 * batch * n
    d_w, d_w2, d_z = dev.to_device(canary(0, words + 16)), dev.to_device(canary(1, words + 16)), dd.filled(2 * batch * (n // 2) + 16)
    W, W2, Z, st = d_w.data_ptr(), d_w2.data_ptr(), d_z.data_ptr(), dev.stream
    enc = lambda z, slots, sc, out, bt, count, form: ck.encode(z, slots, sc, out, bt, count, form, st)      # noqa: E731
    dec = lambda x, form, count, sc, z, slots, scr, bt: ck.decode(x, form, count, sc, z, slots, scr, bt, st)      # noqa: E731
    bad_encode = [(Z, s, scale, W, batch, 0, COEFF), (Z, s, scale, W, batch, 4, COEFF), (Z, 0, scale, W, batch, 3, COEFF), (Z, 3, scale, W, batch, 3, NTT),
                  (Z, n, scale, W, batch, 3, COEFF), (Z, s, 0.0, W, batch, 3, COEFF), (Z, s, -1.0, W, batch, 3, COEFF), (Z, s, math.nan, W, batch, 3, NTT),
                  (Z, s, math.inf, W, batch, 3, COEFF), (Z, s, scale, W, batch, 3, 7), (Z + 4, s, scale, W, batch, 3, COEFF), (Z, s, scale, W + 4, batch, 3, COEFF),
                  (Z, s, scale, W, 1 << 31, 3, COEFF), (Z, s, scale, W, 1 << 55, 3, NTT), (W + 8 * n, s, scale, W, batch, 3, COEFF), (W, s, scale, W, batch, 1, NTT)]
    for args in bad_encode:
        assert status_of(agx, enc, *args) == 5, args
    bad_decode = [(W, COEFF, 0, scale, Z, s, None, batch), (W, NTT, 4, scale, Z, s, W2, batch), (W, COEFF, 3, scale, Z, 5, None, batch), (W, NTT, 3, scale, Z, 64, W2, batch),
                  (W, COEFF, 3, -2.0, Z, s, None, batch), (W, NTT, 3, math.nan, Z, s, W2, batch), (W, 2, 3, scale, Z, s, W2, batch), (W + 4, COEFF, 3, scale, Z, s, None, batch),
                  (W, COEFF, 3, scale, Z + 4, s, None, batch), (W, NTT, 3, scale, Z, s, W2 + 4, batch), (W, COEFF, 3, scale, Z, s, None, 1 << 31),
                  (W, COEFF, 3, scale, W + 8, s, None, batch), (W, NTT, 3, scale, W2 + 16, s, W2, batch), (W, NTT, 3, scale, Z, s, W + 8 * n, batch)]
    for args in bad_decode:
        assert status_of(agx, dec, *args) == 5, args
    assert status_of(agx, dec, W, NTT, 3, scale, Z, s, None, batch) == 1      # NTT form needs its scratch
    assert status_of(agx, enc, Z, s, scale, W, 0, 3, NTT) == 0 and status_of(agx, dec, W, NTT, 3, scale, Z, s, W2, 0) == 0      # batch 0: nothing launched
    assert status_of(agx, dec, W, COEFF, 3, scale, Z, s, W + 8, batch) == 0      # coefficient form never looks at the scratch ...
    assert status_of(agx, dec, W, COEFF, 3, scale, Z, s, W2 + 4, batch) == 0 and status_of(agx, dec, W, COEFF, 3, scale, Z, s, None, batch) == 0      # ... misaligned or NULL
    dev.sync()
    assert np.array_equal(dev.to_host(d_w), canary(0, words + 16)) and np.array_equal(dev.to_host(d_w2), canary(1, words + 16))
    assert np.all(dd.get(d_z)[2 * batch * s:] == -7.25), "the guard band behind d_z was written"      # ... and wrote the slots of its one legal call only
    ck.close()
    # a plan without inverse tables: NTT-form decode says so, after every argument rule; the coefficient form and encode serve
    ck = agx.Ckks(twice, 0, 2)
    d_z = dd.filled(2 * batch * s)
    assert status_of(agx, lambda: ck.decode(W, NTT, 2, scale, d_z.data_ptr(), s, W2, batch, st)) == 9
    assert status_of(agx, lambda: ck.decode(W, NTT, 2, -1.0, d_z.data_ptr(), s, W2, batch, st)) == 5
    dev.sync()
    assert np.all(dd.get(d_z) == -7.25) and np.array_equal(dev.to_host(d_w2), canary(1, words + 16))
    assert status_of(agx, lambda: ck.encode(d_z.data_ptr(), s, scale, W2, batch, 2, NTT, st)) == 0
    ck.close()
    twice.close()
    plan.close()


def test_capture_into_a_graph_and_replay(agx, orc, dev):
    n, s, batch, L, scale = 4096, 2048, 3, 2, 2.0 ** 40
    moduli = tuple(agx.find_primes(60, n, L))
    plan = agx.Plan(n, list(moduli))
    ck, dd = plan.ckks(0, L), Doubles(dev)
    z = _slots(s, batch, 31, False)
    d_z, d_x, d_back = dd.put(z), dev.empty(L * batch * n), dd.filled(2 * batch * s)

    def body(stream):
        ck.encode(d_z.data_ptr(), s, scale, d_x.data_ptr(), batch, L, NTT, stream)
        ck.decode(d_x.data_ptr(), NTT, L, scale, d_back.data_ptr(), s, d_x.data_ptr(), batch, stream)

    graph = capture(dev, body, body)
    want = ref.decode(ref.encode(z, n, moduli, scale), n, moduli, scale, s)
    for _ in range(2):
        d_back.fill_(-7.25)
        graph.replay()
        _same_doubles(dd.get(d_back).view(np.complex128).reshape(batch, s), want, "replay")
    ck.close()
    plan.close()


def test_the_plans_device_must_be_current(agx, orc, dev):
    """with a second GPU: the other device current, both calls answer AGX_ERR_BAD_ARGUMENT and write nothing.  With one GPU (every test machine so far) no
    other device can be made current, so the rule cannot be broken and nothing is checked here"""
    if agx.device_count() < 2:
        return
    torch, n, s, batch, scale = dev.torch, 64, 8, 2, 2.0 ** 30
    plan = agx.Plan(n, list(agx.find_primes(60, n, 2)))
    ck, dd = plan.ckks(0, 2), Doubles(dev)
    d_w, d_z = dev.to_device(canary(0, 2 * batch * n)), dd.filled(2 * batch * s)
    try:
        torch.cuda.set_device(1)
        assert status_of(agx, lambda: ck.encode(d_z.data_ptr(), s, scale, d_w.data_ptr(), batch, 2, COEFF, 0)) == 5
        assert status_of(agx, lambda: ck.decode(d_w.data_ptr(), COEFF, 2, scale, d_z.data_ptr(), s, None, batch, 0)) == 5
        assert status_of(agx, lambda: agx.Ckks(plan, 0, 2).close()) == 5
    finally:
        torch.cuda.set_device(0)
    assert np.array_equal(dev.to_host(d_w), canary(0, 2 * batch * n)) and np.all(dd.get(d_z) == -7.25)
    ck.close()
    plan.close()


def test_one_encrypted_run_end_to_end(agx, orc, dev):
    """INTEGRATION.md's CKKS listing at n = 64, batch 2, full slots, Delta = 2^40, Q = (60, 60, 40 bits), two 60-bit special primes: encode; symmetric encryption
    with a (uniform) and e (cbd 21) drawn by the sampling calls under a ternary secret of weight 8; multiply by an encoded plaintext; agx_ntt_rescale by the 40-bit
    prime on the plan of the three primes of Q; one hoisted rotation by r = 1 at level 2 (decompose, apply_decomposed with the noise-free key of
    rns_ref.rotation_key_case, sigma_g(c_0) by add_galois); decryption; decode at Delta^2 / q_last with count = 2, a prefix of the handle.  The result is
    z o w rotated left by 1 within a tolerance the test computes from what it sampled.  In the coefficients of the phase: e W / q_last, at most
    |e|_inf |W|_1 / q_last; the rescale's two roundings, (1 + |s|_1) / 2; the key switch, p_count (1 + |s|_1) (rotation_bound); a coefficient error eps costs
    the slots at most n |eps|_inf / Delta'.  To that come the decode bound and the two encode roundings carried to the slots as in the product test."""
    n, batch, r = 64, 2, 1
    s_count, scale = n // 2, 2.0 ** 40
    moduli = moduli_for(orc.find_prime, n, [60, 60, 40, 60, 60])
    Q3, Q2, q_last = moduli[:3], moduli[:2], moduli[2]
    shape = (2, 3, 2, 2)      # the key switch at level 2: Q = primes [0, 2), special primes [3, 5), one digit
    g = agx.galois_element(n, r)
    plan, _ = plan_for_moduli(agx, orc, n, moduli)
    plan3, _ = plan_for_moduli(agx, orc, n, Q3)      # agx_ntt_rescale divides by its plan's last prime
    _, key, sec, _ = rotation_key_case(orc, n, moduli, shape, g, batch, 4242)
    shat3 = oracle_forward_set(orc, n, Q3, np.stack([(sec % int(q)).astype(np.uint64) for q in Q3]))      # [3][n]: one frame per prime
    ck, dd, st = plan.ckks(0, 3), Doubles(dev), dev.stream
    slab, seed = batch * n, bytes(range(32))
    z, w = _slots(s_count, batch, 41, False), _slots(s_count, batch, 42, False)
    d_shat = dev.to_device(shat3.reshape(-1))
    d_c0, d_c1, d_e, d_as, d_w = (dev.empty(3 * slab) for _ in range(5))
    # encode and encrypt: c_1 = a, c_0 = m - a s + e
    ck.encode(dd.put(z).data_ptr(), s_count, scale, d_c0.data_ptr(), batch, 3, NTT, st)
    plan.sample_uniform(seed, 1, d_c1.data_ptr(), batch, 0, 0, 3, st)
    plan.sample_cbd(seed, 1, 21, d_e.data_ptr(), batch, 0, 0, 3, NTT, st)
    plan.mul_add_galois(d_shat.data_ptr(), d_c1.data_ptr(), d_as.data_ptr(), batch, 1, 1, False, 0, 3, st)
    plan.sub(d_c0.data_ptr(), d_as.data_ptr(), d_c0.data_ptr(), batch, 0, 3, st)
    plan.add(d_c0.data_ptr(), d_e.data_ptr(), d_c0.data_ptr(), batch, 0, 3, st)
    # multiply by the encoded plaintext w: both components, frame by frame; the scale becomes Delta^2
    ck.encode(dd.put(w).data_ptr(), s_count, scale, d_w.data_ptr(), batch, 3, NTT, st)
    for d_c in (d_c0, d_c1):
        plan.mul_add_galois(d_w.data_ptr(), d_c.data_ptr(), d_c.data_ptr(), batch, 1, None, False, 0, 3, st)
    # rescale: level 3 -> 2, the scale Delta^2 / q_last
    d_r0, d_r1, d_scr = dev.empty(2 * slab), dev.empty(2 * slab), dev.empty(slab)
    for d_c, d_r in ((d_c0, d_r0), (d_c1, d_r1)):
        plan3.rescale(d_c.data_ptr(), d_r.data_ptr(), d_scr.data_ptr(), batch, agx.RESCALE_ROUND, st)
    # rotate left by r: (sigma_g(c_0) + out_0, out_1) with (out_0, out_1) the hoisted key switch of c_1 under g
    ks = plan.keyswitch(*shape)
    ext_words, dscr_words, ascr_words = ks.hoisted_words(batch)
    d_ext, d_ds, d_as2, d_key, d_out = dev.empty(ext_words), dev.empty(dscr_words), dev.empty(ascr_words), dev.to_device(key.reshape(-1)), dev.empty(2 * 2 * slab)
    ks.decompose(d_r1.data_ptr(), d_ext.data_ptr(), d_ds.data_ptr(), batch, st)
    ks.apply_decomposed(d_ext.data_ptr(), d_key.data_ptr(), d_out.data_ptr(), d_as2.data_ptr(), batch, g, st)
    d_phase = dev.empty(2 * slab)
    plan.add_galois(d_out.data_ptr(), d_r0.data_ptr(), d_phase.data_ptr(), batch, g, 0, 2, st)
    # decrypt: c_0 + c_1 s on the two primes of the level (the first two slabs of the secret), then decode with a scratch of its own
    plan.mul_add_galois(d_shat.data_ptr(), d_out.data_ptr() + 8 * 2 * slab, d_phase.data_ptr(), batch, 1, 1, True, 0, 2, st)
    phase = dev.to_host(d_phase).reshape(2, batch, n)
    scale2 = scale * scale / float(q_last)
    d_back, d_scratch = dd.filled(2 * batch * s_count), dev.empty(2 * slab)
    ck.decode(d_phase.data_ptr(), NTT, 2, scale2, d_back.data_ptr(), s_count, d_scratch.data_ptr(), batch, st)
    got = dd.get(d_back).view(np.complex128).reshape(batch, s_count)
    # the tolerance, from what was sampled
    e = ref.centred(oracle_inverse_set(orc, n, Q3, dev.to_host(d_e).reshape(3, -1)).tolist(), Q3)
    e_inf, s_one = max(abs(v) for v in e), int(np.abs(sec).sum())
    assert 0 < e_inf <= 21 and s_one == 8
    W = ref.encode_integers(w, n, scale)
    coeffs = oracle_inverse_set(orc, n, Q2, phase).reshape(2, batch, n)
    for f in range(batch):
        eps = e_inf * sum(abs(v) for v in W[f]) / q_last + (1 + s_one) / 2 + rotation_bound(shape, sec)
        r1 = (2 * s_count) * (0.5 + _encode_slack(z[f], s_count, scale)) / scale
        r2 = (2 * s_count) * (0.5 + _encode_slack(w[f], s_count, scale)) / scale
        X = ref.centred([coeffs[i][f].tolist() for i in range(2)], Q2)
        tol = _decode_bound(X, s_count, 2, scale2) + n * eps / scale2 + r1 * float(np.abs(w[f]).max()) + r2 * float(np.abs(z[f]).max()) + r1 * r2
        err = float(np.abs(got[f] - np.roll(z[f] * w[f], -r)).max())
        print("encrypted run, frame", f, "error", err, "tolerance", tol, "of which noise", n * eps / scale2)
        assert err <= tol, (f, err, tol)
        assert float(np.abs(got[f] - z[f] * w[f]).max()) > 1e-3      # the rotation moved the slots
    ks.close()
    ck.close()
    plan3.close()
    plan.close()
