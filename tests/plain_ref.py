"""The Python-integer reference model of agx_ntt_plain_scale_up, _lift and _scale_down (BFV's plaintext boundary; include/agx_ntt.h has the contract):
the three formulas exactly as the header states them, the (h - rho) t^-1 form the device uses for scale_up, and the rounding property of scale_down.  Python
integers and nothing else beside bfv_conv_ref.py (product, centre).  The GPU tests are judged against this module; this module is judged on the CPU by
tests/test_plain_reference.py.

A frame set is a list [len(Q)][count] of integers, row i under Q[i]; a plaintext is a list [count].  Any words are reduced before they are used."""
from bfv_conv_ref import centre, negacyclic, product


def scale_up(m, Q, t):
    """m [count] (any words) -> [L][count]: U mod q_i with U = floor((2 D m' + t) / (2t)), m' = m mod t"""
    D = product(Q)
    U = [(2 * D * (v % t) + t) // (2 * t) for v in m]
    return [[u % q for u in U] for q in Q]


def scale_up_device_form(m, Q, t):
    """the same words by rho = ((D mod t) m' + h) mod t and U mod q_i = (h - rho) t^-1 mod q_i"""
    D, h = product(Q), t // 2
    rho = [((D % t) * (v % t) + h) % t for v in m]
    return [[(h - r) * pow(t, -1, q) % q for r in rho] for q in Q]


def lift(m, Q, t):
    """m [count] (any words) -> [L][count]: m' mod q_i for m' < ceil(t / 2), (m' - t) mod q_i from there on"""
    half = (t + 1) // 2
    c = [v % t if v % t < half else v % t - t for v in m]
    return [[v % q for v in c] for q in Q]


def scale_down_parts(x, Q, gamma, t):
    """x [L][count] (any words) -> per coefficient (V, s_t, s_gamma, c, m), the words of the header's formula"""
    D = product(Q)
    w = [gamma * t * pow(D // q, -1, q) % q for q in Q]      # gamma t Q_i^-1 mod q_i
    d_t, d_g, g_t = pow(D, -1, t), pow(D, -1, gamma), pow(gamma, -1, t)
    out = []
    for e in range(len(x[0])):
        V = sum((int(xi[e]) % q) * wi % q * (D // q) for xi, q, wi in zip(x, Q, w))
        s_t = -V * d_t % t
        s_g = -V * d_g % gamma
        c = centre(s_g, gamma)
        out.append((V, s_t, s_g, c, (s_t - c) * g_t % t))
    return out


def scale_down(x, Q, gamma, t):
    """x [L][count] (any words) -> [count] in [0, t): the formula, defined for every input"""
    return [p[4] for p in scale_down_parts(x, Q, gamma, t)]


def residues(X, Q):
    """the integers X [count] -> [L][count]"""
    return [[v % q for v in X] for q in Q]


def phase(ct, s, Q):
    """the residues [L][n] of c_0 + c_1 s (+ c_2 s^2) mod (X^n + 1, q_i): what decryption rounds; ct has two or three components, each [L][n]"""
    rows = []
    for j, q in enumerate(Q):
        sq = [v % q for v in s]
        row, power = [v % q for v in ct[0][j]], sq
        for c in ct[1:]:
            row = [(u + v) % q for u, v in zip(row, negacyclic(c[j], power, q))]
            power = negacyclic(power, sq, q)
        rows.append(row)
    return rows


def within_margin(X, Q, gamma, t):
    """per integer X: does t X / D = R + f, R the nearest integer (halves up), have |f| <= 1/2 - L / gamma?  Exact, in integers: with N = 2 t X + D and
    R = N // (2 D), f = (t X - R D) / D, so the test is gamma |t X - R D| <= (gamma - 2 L) D / 2, i.e. 2 gamma |t X - R D| <= (gamma - 2 L) D"""
    D, L = product(Q), len(Q)
    return [2 * gamma * abs(t * v - ((2 * t * v + D) // (2 * D)) * D) <= (gamma - 2 * L) * D for v in X]


def rounded(X, Q, t):
    """(2 t X + D) // (2 D) % t per integer X: round(t X / D) mod t, halves up"""
    D = product(Q)
    return [(2 * t * v + D) // (2 * D) % t for v in X]
