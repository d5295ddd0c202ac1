"""tests/plain_ref.py, the Python-integer model of agx_ntt_plain_scale_up / _lift / _scale_down, judged on the CPU: U equals its (h - rho) t^-1 form; the lift
is the centred representative; scale_down equals (2 t X + D) // (2 D) % t on every coefficient that meets |f| <= 1/2 - L / gamma, and the fixed seeds below
exclude none (asserted, not skipped); scale_down decrypts what bfv_conv_ref.encrypt and bfv_conv_ref.multiply produce, as bfv_conv_ref.decrypt does;
scale_down(scale_up(m) + e) == m for small e; t in {2, 3, 65536, 65537, 2^61 - 1}, including t above every q_i."""
import pytest

import bfv_conv_ref as ref
import plain_ref as pref
from modulus_cases import prime_below

T_VALUES = (2, 3, 65536, 65537, (1 << 61) - 1)      # 2^61 - 1 is odd (a Mersenne prime) and above every modulus of the first two sets
# (widths of Q, width of gamma) at n = 64: a small Q that every t but the first two exceeds; the BFV set; a wide one; L = 1
SETS = (((30, 31), 50), ((45, 52), 60), ((60, 61, 62, 54), 59), ((58,), 45))
COUNT = 750      # coefficients per (set, t): 4 x 5 x 750 = 15,000, and the BFV tests besides


def _moduli(orc, widths, gamma_bits, n=64):
    seen, Q = {}, []
    for b in widths:
        Q.append(prime_below(orc, 1 << b, n, seen.get(b, 0)))
        seen[b] = seen.get(b, 0) + 1
    gamma = prime_below(orc, 1 << gamma_bits, n, 3)      # away from every prime of Q of the same width
    assert gamma not in Q and gamma >= 1 << 44
    return tuple(Q), gamma


def _usable(Q, gamma, t):
    return all(t % q for q in Q) and t % gamma


@pytest.mark.parametrize("t", T_VALUES)
@pytest.mark.parametrize("widths,gamma_bits", SETS, ids=str)
def test_scale_up_is_its_device_form_and_lift_is_centred(orc, widths, gamma_bits, t):
    Q, gamma = _moduli(orc, widths, gamma_bits)
    assert _usable(Q, gamma, t)
    rng = ref.Rng(t + sum(widths))
    m = [0, 1, t - 1, t, t // 2, t // 2 + 1, (t + 1) // 2 - 1, (t + 1) // 2, 2**64 - 1, 2**63] + [rng.below(2**64) for _ in range(COUNT)]
    up = pref.scale_up(m, Q, t)
    assert up == pref.scale_up_device_form(m, Q, t)
    D = ref.product(Q)
    for e, v in enumerate(m):      # U is D m' / t rounded, halves up
        U = (2 * D * (v % t) + t) // (2 * t)
        assert 2 * abs(U * t - D * (v % t)) <= t and [U % q for q in Q] == [row[e] for row in up]
    lifted = pref.lift(m, Q, t)
    for e, v in enumerate(m):
        c = ref.crt_centred([[row[e]] for row in lifted], Q)[0] if D > 2 * t else None
        want = v % t if 2 * (v % t) < t else v % t - t
        assert -t // 2 <= want <= (t - 1) // 2 and (want - v) % t == 0
        assert c is None or c == want
        assert [want % q for q in Q] == [row[e] for row in lifted]


@pytest.mark.parametrize("t", T_VALUES)
@pytest.mark.parametrize("widths,gamma_bits", SETS, ids=str)
def test_scale_down_rounds_wherever_the_margin_holds(orc, widths, gamma_bits, t):
    """X uniform below D, and X built next to the rounding boundary on either side; no coefficient of these seeds falls outside the margin"""
    Q, gamma = _moduli(orc, widths, gamma_bits)
    D, L = ref.product(Q), len(Q)
    rng = ref.Rng(7 * t + gamma_bits)
    X = [0, 1, D - 1, D // t, D // t + 1] + [rng.below(D) for _ in range(COUNT)]      # not D // 2: with an odd t that is a tie, t X / D = t / 2 - t / (2 D)
    if D > 4 * t * gamma:
        # t X / D = R + f with f just inside the margin: X = ceil((R + f) D / t) - or floor -, f = +-(1/2 - (L + 1) / gamma)
        for _ in range(64):
            R = rng.below(min(t, D // t))
            num = R * 2 * gamma + (gamma - 2 * (L + 1))      # (R + 1/2 - (L + 1) / gamma) 2 gamma
            X += [num * D // (2 * gamma * t), -(-(num - 2 * (gamma - 2 * (L + 1))) * D // (2 * gamma * t))]
    inside = pref.within_margin(X, Q, gamma, t)
    assert all(inside), ("the model excludes coefficients", inside.count(False))
    assert pref.scale_down(pref.residues(X, Q), Q, gamma, t) == pref.rounded(X, Q, t)
    # any representative with those residues, negative ones included, and lazy words
    shifted = [v - D * (k % 3) for k, v in enumerate(X)]
    lazy = [[v + q * (k % 4) for k, v in enumerate(row)] for row, q in zip(pref.residues(shifted, Q), Q)]
    assert pref.scale_down(lazy, Q, gamma, t) == pref.rounded(X, Q, t)


@pytest.mark.parametrize("t", T_VALUES)
def test_scale_down_of_scale_up_plus_small_noise_is_the_message(orc, t):
    Q, gamma = _moduli(orc, (45, 52), 60)
    rng = ref.Rng(t)
    m = [0, 1, t - 1, t // 2] + [rng.below(t) for _ in range(COUNT)]
    up = pref.scale_up(m, Q, t)
    for noise in (0, 1, 1 << 20):
        e = [rng.below(2 * noise + 1) - noise for _ in m]
        x = [[(u + ee) % q for u, ee in zip(row, e)] for row, q in zip(up, Q)]
        assert pref.scale_down(x, Q, gamma, t) == m, noise


def _bfv(orc, n):
    w = ref.BFV_WIDTHS
    Q = tuple(prime_below(orc, 1 << b, n) for b in w["Q"])
    B = tuple(prime_below(orc, 1 << b, n) for b in w["B"])
    return Q, B, prime_below(orc, 1 << w["m_sk"], n), prime_below(orc, 1 << w["m_tilde"], n), ref.BFV_T


def test_scale_down_decrypts_as_the_big_integer_division_does(orc):
    """BFV_WIDTHS, BFV_T, gamma = each prime of B: fresh ciphertexts and the three-component output of a multiplication"""
    n = 16
    Q, B, m_sk, m_tilde, t = _bfv(orc, n)
    rng = ref.Rng(61)
    s = ref.keygen(rng, n)
    msgs = [[rng.below(t) for _ in range(n)] for _ in range(2)]
    cts = [ref.encrypt(rng, msg, s, Q, t) for msg in msgs]
    product = ref.multiply(cts[0], cts[1], Q, B, m_sk, m_tilde, t)["out"]
    for gamma in B:
        for ct, want in ((cts[0], msgs[0]), (cts[1], msgs[1]), (product, ref.negacyclic(msgs[0], msgs[1], t))):
            assert ref.decrypt(ct, s, Q, t) == want
            assert pref.scale_down(pref.phase(ct, s, Q), Q, gamma, t) == want
    # encryption from scale_up: c_0 = U - a s + e decrypts to the message too (U = D m / t rounded, where encrypt takes floor(D / t) m)
    up = pref.scale_up(msgs[0], Q, t)
    a = [rng.below(ref.product(Q)) for _ in range(n)]
    e = [rng.below(17) - 8 for _ in range(n)]
    c0 = [[(u - w + ee) % q for u, w, ee in zip(row, ref.negacyclic([v % q for v in a], [v % q for v in s], q), e)] for row, q in zip(up, Q)]
    ct = [c0, [[v % q for v in a] for q in Q]]
    assert ref.decrypt(ct, s, Q, t) == msgs[0] and pref.scale_down(pref.phase(ct, s, Q), Q, B[0], t) == msgs[0]


def test_the_formula_is_defined_where_the_property_does_not_hold(orc):
    """tiny moduli and a tiny gamma: every word in range, s_gamma takes both centring edges, and m (s.t. gamma m = s_t - c mod t) is what the parts say"""
    Q, gamma = (97, 113), 17      # admitted at n = 8
    for t in (2, 5, 65536):
        x = [[a for a in range(97) for _ in range(113)], [b for _ in range(97) for b in range(113)]]
        parts = pref.scale_down_parts(x, Q, gamma, t)
        assert {p[2] for p in parts} == set(range(gamma)) and {(gamma - 1) // 2, (gamma + 1) // 2} <= {p[2] for p in parts}
        assert all(0 <= p[4] < t and (p[4] * gamma - p[1] + p[3]) % t == 0 and abs(p[3]) <= (gamma - 1) // 2 for p in parts)
