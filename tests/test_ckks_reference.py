"""The float64 model of agx_ntt_ckks_encode / _decode (tests/ckks_ref.py) judged on the CPU: every twiddle against mpmath; the model against the closed
forms in high precision (exact_*) under the two derived bounds of the issue, with the observed share of each bound printed per case
(profiles/r20_ckks_boundary.md records them); the condition that makes the GPU accuracy test meaningful (the exact-equality class holds at least 99 % of the
coefficients wherever Delta <= 2^40); Garner's digits, sign and magnitude against Python integers at the edges; and the properties of the model: rotation,
conjugation, the round trip and the product.

Bounds, with t = log2(2s), u = 2^-53 and |.| the 2-norm (Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2, with eta <= 8u for twiddles within
one ulp, plus the Horner and scaling roundings):
    decode  |z_j - exact| <= (8t + 4l + 2) u sqrt(s) |X| / Delta
    encode  |c_k - Delta w_k| <= 1/2 + E,  E = (8t + 2) u Delta |z| / sqrt(s);  c_k = rint(Delta w_k) wherever Delta w_k is farther than E from a half-integer."""
import math

import numpy as np
import pytest

import ckks_ref as ref

U = 2.0 ** -53
SIZES = (2, 8, 64, 1024, 4096)


def _primes(agx, n, count, bits=60):
    return tuple(agx.find_primes(bits, n, count))


def _slots(s, batch, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (batch, s)) + 1j * rng.uniform(-1, 1, (batch, s))) / math.sqrt(2)


def _samples(s, limit=6):
    return list(range(s)) if s <= 32 else sorted({0, 1, s // 2, s - 1, 5, (s // 3) | 1})[:limit]


def test_every_twiddle_is_within_2_to_minus_53_of_the_real_value(agx):
    """tw(len, j) sits at the angle 2 pi r / (4 len), r = 5^j mod 4 len: the root zeta'^r of s = len in the reference's table (mpmath at 200 bits; without it
    longdouble from an exact octant reduction, whose own error of 2^-63 is allowed for)"""
    worst, length = 0.0, 2
    own = 0.0 if ref.mpmath is not None else 2.0 ** -62
    while length <= 16384:
        r = 1
        for j in range(length // 2):
            c, s = agx.ckks_twiddle(length, j)
            re, im = ref.root(length, r)
            worst = max(worst, ref.distance(c, re), ref.distance(s, im))
            r = r * 5 % (4 * length)
        length *= 2
    print("largest twiddle error", worst, "in units of 2^-53:", worst / U)
    assert worst <= U + own


@pytest.mark.parametrize("n", SIZES)
def test_the_model_against_the_closed_forms(agx, n):
    ratios = []
    for s in sorted({n // 2, max(1, n // 8), 1}):
        for L, scale in ((2, 2.0 ** 40), (1, 2.0 ** 30)):
            Q = _primes(agx, n, L)
            t = math.log2(2 * s)
            z = _slots(s, 1, 1000 + n + s)
            c = ref.encode_integers(z, n, scale)[0]
            gap = (n // 2) // s
            ks = _samples(s)
            E = (8 * t + 2) * U * scale * float(np.linalg.norm(z[0])) / math.sqrt(s)
            exact = ref.exact_encode(z[0], s, ks)
            worst_e = 0.0
            for k in ks:
                for idx, part in ((k * gap, exact[k].real), ((k + s) * gap, exact[k].imag)):
                    target = ref.scaled(scale, part)
                    err = ref.distance(c[idx], target)
                    assert err <= 0.5 + E, (n, s, idx, err, E)
                    nearest, margin = ref.nearest_and_margin(target)
                    if margin > E:
                        assert c[idx] == nearest, (n, s, idx)
                    worst_e = max(worst_e, max(0.0, err - 0.5) / E)
            assert all(v == 0 for i, v in enumerate(c) if i % gap)      # off the gap grid
            x = np.array([[[v % q for v in c]] for q in Q], dtype=np.uint64)
            got = ref.decode(x, n, Q, scale, s)[0]
            bound = (8 * t + 4 * L + 2) * U * math.sqrt(s) * math.sqrt(sum(float(v) ** 2 for v in c)) / scale
            zz = ref.exact_decode(c, n, s, scale, ks)
            worst_d = max(max(ref.distance(got[j].real, zz[j].real), ref.distance(got[j].imag, zz[j].imag)) for j in ks)
            assert worst_d <= bound, (n, s, worst_d, bound)
            ratios.append((n, s, L, int(math.log2(scale)), worst_e, worst_d / bound if bound else 0.0))
    for r in ratios:
        print("n %5d s %5d l %d Delta 2^%d: encode excess / E %.4f, decode error / bound %.4f" % r)


@pytest.mark.parametrize("n,scale,frames", [(64, 2.0 ** 40, 32), (4096, 2.0 ** 30, 1), (32768, 2.0 ** 30, 1)])
def test_the_exact_equality_class_holds_nearly_every_coefficient(agx, n, scale, frames):
    """the condition behind the GPU accuracy cases (Delta <= 2^40): at least 99 % of the coefficients lie farther than E from a half-integer.  At n = 64 every
    coefficient of 32 frames is classed by its exact value, and the model's double x is held to lie within E of it; at the large sizes the model's x is classed
    itself: it lies within E of the exact value (the bound above), so a margin of x above 2E implies a margin of the exact value above E"""
    s = n // 2
    t = math.log2(2 * s)
    z = _slots(s, frames, 11 if frames == 1 else 77)
    inside = total = 0
    for f in range(frames):
        E = (8 * t + 2) * U * scale * float(np.linalg.norm(z[f])) / math.sqrt(s)
        re, im = ref.fft_inverse(z[f:f + 1].real.copy(), z[f:f + 1].imag.copy())
        x = np.concatenate([scale * (re[0] * (1.0 / s)), scale * (im[0] * (1.0 / s))])      # the model's own doubles, before the rounding
        if n <= 64:
            exact = ref.exact_encode(z[f], s, range(s))
            parts = [exact[k].real for k in range(s)] + [exact[k].imag for k in range(s)]
            for xk, part in zip(x.tolist(), parts):
                target = ref.scaled(scale, part)
                assert ref.distance(xk, target) <= E      # the model's x lies within E of the exact value ...
                inside += ref.nearest_and_margin(target)[1] > E      # ... so in this class its rounding is the exact value's
                total += 1
        else:
            inside += int(np.sum(np.abs(x - np.floor(x) - 0.5) > 2 * E))
            total += x.size
    print("n", n, "Delta 2^%d" % int(math.log2(scale)), "share in the exact-equality class", inside / total)
    assert inside >= 0.99 * total, (inside, total)


@pytest.mark.parametrize("L", [1, 2, 3, 16])
def test_garner_digits_sign_and_magnitude_at_the_edges(agx, L):
    n = 64
    Q = _primes(agx, n, L) if L < 16 else _primes(agx, n, 8) + _primes(agx, n, 4, 31) + _primes(agx, n, 4, 20)
    D = math.prod(Q)
    half = (D - 1) // 2
    values = [0, 1, -1, half, -half, half - 1, -half + 1]
    part = 1
    for q in Q[:-1]:      # a carry through every digit below: -(q_0 ... q_i) has the magnitude digits 0, ..., 0, 1
        part *= q
        if part <= half:
            values += [part, -part, -part + 1, -part - 1]
    rng = np.random.default_rng(L)
    values += [int(v) % D - half for v in rng.integers(0, 2 ** 63, size=50, dtype=np.uint64).astype(object) ** 3]
    for X in values:
        x = [X % q for q in Q]
        v = ref.garner_digits(x, Q)
        rest, digits = X % D, []
        for q in Q:
            digits.append(rest % q)
            rest //= q
        assert v == digits, X
        negative, w = ref.centred_digits(v, Q)
        assert negative == (X < 0), X
        mag, place = 0, 1
        for d, q in zip(w, Q):
            assert 0 <= d < q
            mag, place = mag + d * place, place * q
        assert mag == abs(X), X
        got = ref.rns_to_double(x, Q)
        assert got == float(X) or abs(got - X) <= abs(X) * 2 * L * U, (X, got)      # one rounding per Horner step
        if abs(X) < 2 ** 53:
            assert got == float(X)


@pytest.mark.parametrize("n,s", [(8, 4), (64, 32), (64, 8), (1024, 512)])
def test_properties_of_the_model(agx, n, s):
    """rotation by 5^r and conjugation by 2n - 1 permute the slots as the header says (full slots), decode(encode z) = z and the product of two encodings
    decodes to z o z' at scale Delta^2, each within the decode bound plus the encode rounding carried to the slots"""
    Q, scale = _primes(agx, n, 3), 2.0 ** 40
    D = math.prod(Q)
    z, z2 = _slots(s, 1, 5), _slots(s, 1, 6)
    c, c2 = ref.encode_integers(z, n, scale)[0], ref.encode_integers(z2, n, scale)[0]
    t = math.log2(2 * s)
    rounding = (2 * s) * (0.5 + (8 * t + 2) * U * scale * float(np.linalg.norm(z[0])) / math.sqrt(s)) / scale

    def decoded(X, sc):
        x = np.array([[[v % q for v in X]] for q in Q], dtype=np.uint64)
        bound = (8 * t + 4 * len(Q) + 2) * U * math.sqrt(s) * math.sqrt(sum(float(v) ** 2 for v in X)) / sc
        return ref.decode(x, n, Q, sc, s)[0], bound

    got, bound = decoded(c, scale)
    assert np.abs(got - z[0]).max() <= bound + rounding
    if s == n // 2:
        for g, want in [(pow(5, r, 2 * n), np.roll(z[0], -r)) for r in (1, 3)] + [(2 * n - 1, np.conj(z[0]))]:
            rotated = [0] * n      # a(X) -> a(X^g) modulo X^n + 1
            for i, v in enumerate(c):
                e = i * g % (2 * n)
                rotated[e % n] = v if e < n else -v
            got, bound = decoded(rotated, scale)
            assert np.abs(got - want).max() <= bound + rounding, g
    prod = [0] * n      # the negacyclic product
    for i, a in enumerate(c):
        if a:
            for j, b in enumerate(c2):
                k = i + j
                prod[k % n] += a * b if k < n else -a * b
    assert max(abs(v) for v in prod) < D // 2
    got, bound = decoded(prod, scale * scale)
    rounding2 = (2 * s) * (0.5 + (8 * t + 2) * U * scale * float(np.linalg.norm(z2[0])) / math.sqrt(s)) / scale
    assert np.abs(got - z[0] * z2[0]).max() <= bound + rounding * float(np.abs(z2).max()) + rounding2 * float(np.abs(z).max()) + rounding * rounding2
