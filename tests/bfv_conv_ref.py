"""The Python-integer reference model of the two exact base conversions of a BFV multiplication (BEHZ: Bajard, Eynard, Hasan, Zucca, SAC 2016):
agx_ntt_basis_extend_exact (Shenoy-Kumaresan) and agx_ntt_basis_extend_mont (FastBConv_m~ followed by the small Montgomery reduction), the approximate
conversion and ModDown beside them, and a whole BFV multiplication by the seven steps of INTEGRATION.md, "BFV multiplication (BEHZ)", with the transforms
replaced by schoolbook negacyclic products.  Python integers and nothing else: it imports nothing.  The GPU tests are judged against this module; this
module is judged on the CPU by tests/test_bfv_conv_reference.py.

A frame set is a list [len(moduli)][count] of integers, row i under moduli[i]; any words are reduced below their modulus before they are used, so words
spread over the lazy range [0, 4q) are the same inputs as their residues."""


def product(moduli):
    D = 1
    for q in moduli:
        D *= int(q)
    return D


def centre(a, m):
    """a in [0, m), m odd: a for a <= (m - 1) / 2, a - m above"""
    assert 0 <= a < m and m & 1
    return a if a <= (m - 1) // 2 else a - m


def lift(x, src, scale=1):
    """x [S][count] (any words) -> V = sum_i y_i D_i per coefficient, y_i = x_i scale D_i^-1 mod q_i in [0, q_i); 0 <= V < S D"""
    D = product(src)
    V = [0] * len(x[0])
    for xi, q in zip(x, src):
        Di = D // q
        w = scale * pow(Di, -1, q) % q
        for e, v in enumerate(xi):
            V[e] += (v % q) * w % q * Di
    return V


def extend_approx(x, src, dst):
    """agx_ntt_basis_extend in coefficient form: out_j = V mod q_j, V = X + u D with 0 <= u < S"""
    V = lift(x, src)
    return [[v % q for v in V] for q in dst]


def alpha_exact(x, r, src, m):
    """(V, alpha) per coefficient: alpha = centre(((V - r') D^-1) mod m)"""
    D = product(src)
    V = lift(x, src)
    return V, [centre((v - rr % m) * pow(D, -1, m) % m, m) for v, rr in zip(V, r)]


def extend_exact(x, r, src, dst, m):
    """agx_ntt_basis_extend_exact in coefficient form: x [S][count], r [count] (any words) -> [T][count], out_j = (V - alpha D) mod q_j"""
    D = product(src)
    V, alpha = alpha_exact(x, r, src, m)
    return [[(v - a * D) % q for v, a in zip(V, alpha)] for q in dst]


def mont_value(x, src, m):
    """W = (V + alpha D) / m per coefficient, an exact integer: y_i = x_i' (m D_i^-1) mod q_i, V = sum_i y_i D_i, alpha = centre((-V D^-1) mod m)"""
    D = product(src)
    W = []
    for v in lift(x, src, scale=m):
        num = v + centre(-v * pow(D, -1, m) % m, m) * D
        assert num % m == 0
        W.append(num // m)
    return W


def extend_mont(x, src, dst, m):
    """agx_ntt_basis_extend_mont in coefficient form: x [S][count] (any words) -> [T][count], out_j = W mod q_j = (V + alpha D) m^-1 mod q_j"""
    return [[w % q for w in mont_value(x, src, m)] for q in dst]


def mod_down(a, p, src, dst):
    """agx_ntt_basis_mod_down in coefficient form (FLOOR, t = 1): a [T][count], p [S][count] -> [T][count], out_j = (a_j - V) D^-1 mod q_j"""
    D = product(src)
    V = lift(p, src)
    return [[(v - w) * pow(D, -1, q) % q for v, w in zip(aj, V)] for aj, q in zip(a, dst)]


# ---- polynomials modulo X^n + 1 -----------------------------------------------------------------------------------------------------------
def negacyclic(a, b, q):
    """a b mod (X^n + 1, q), schoolbook"""
    n = len(a)
    c = [0] * n
    for i, u in enumerate(a):
        if u:
            for j, v in enumerate(b):
                if i + j < n:
                    c[i + j] += u * v
                else:
                    c[i + j - n] -= u * v
    return [v % q for v in c]


def crt_centred(x, moduli):
    """x [len(moduli)][count] -> the integers in (-D/2, D/2] with those residues"""
    D = product(moduli)
    X = [0] * len(x[0])
    for xi, q in zip(x, moduli):
        w = (D // q) * pow(D // q, -1, q)
        for e, v in enumerate(xi):
            X[e] += (v % q) * w
    return [v % D - D if v % D > D // 2 else v % D for v in X]


# ---- BFV ----------------------------------------------------------------------------------------------------------------------------------
# The parameter set of the end-to-end tests: widths in bits of Q (L = 2), B (K = 3), m_sk and m~, the largest prime = 1 (mod 2n) below each; t.  Mixed
# widths on purpose: primes that all lie just below 2^60 make B mod Q tiny, and a wrong conversion then still decrypts.
BFV_WIDTHS = {"Q": (45, 52), "B": (60, 57, 54), "m_sk": 59, "m_tilde": 50}
BFV_T = 65537


class Rng:
    """splitmix64: the model's own generator, so that it imports nothing"""

    def __init__(self, seed):
        self.s = seed & (2**64 - 1)

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & (2**64 - 1)
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        return z ^ (z >> 31)

    def below(self, bound):
        return (self.next() << 64 | self.next()) % bound


def keygen(rng, n):
    """a ternary secret"""
    return [rng.below(3) - 1 for _ in range(n)]


def encrypt(rng, msg, s, Q, t, noise=8):
    """(c0, c1), each [L][n]: c1 = a uniform, c0 = floor(Q / t) msg - a s + e with |e| <= noise"""
    n, D = len(msg), product(Q)
    delta = D // t
    a = [rng.below(D) for _ in range(n)]
    e = [rng.below(2 * noise + 1) - noise for _ in range(n)]
    c0, c1 = [], []
    for q in Q:
        as_ = negacyclic([v % q for v in a], [v % q for v in s], q)
        c0.append([(delta * mm - w + ee) % q for mm, w, ee in zip(msg, as_, e)])
        c1.append([v % q for v in a])
    return [c0, c1]


def decrypt(ct, s, Q, t):
    """round(t / Q [sum_k c_k s^k]_Q) mod t per coefficient; ct has two or three components, each [L][n]"""
    D = product(Q)
    acc = []
    for j, q in enumerate(Q):
        sq = [v % q for v in s]
        row, power = list(ct[0][j]), sq
        for c in ct[1:]:
            row = [(u + v) % q for u, v in zip(row, negacyclic(c[j], power, q))]
            power = negacyclic(power, sq, q)
        acc.append(row)
    return [(2 * t * v + D) // (2 * D) % t for v in crt_centred(acc, Q)]


def multiply(ct1, ct2, Q, B, m_sk, m_tilde, t, exact=True):
    """The seven steps of the INTEGRATION.md listing on coefficient-form ciphertexts ct [2][L][n]: {"operands": [2][2][L + K + 1][n] (step 2: the Q rows
    reduced, the Bsk rows from extend_mont), "tensor": [3][L + K + 1][n] (steps 3 and 4: the products times t), "floor": [3][K + 1][n] (step 5 and 6:
    ModDown, sources Q, targets Bsk), "out": [3][L][n] (step 7)}.  exact = False replaces step 7's extend_exact by the approximate conversion."""
    Q, B = tuple(Q), tuple(B)
    Bsk = B + (m_sk,)
    every = Q + Bsk
    L, K = len(Q), len(B)
    operands = [[[[v % q for v in row] for row, q in zip(c, Q)] + extend_mont(c, Q, Bsk, m_tilde) for c in ct] for ct in (ct1, ct2)]      # steps 1, 2
    (a0, a1), (b0, b1) = operands
    tensor = [[], [], []]
    for p, q in enumerate(every):                                                                                                          # steps 3, 4
        cross = [(u + v) % q for u, v in zip(negacyclic(a0[p], b1[p], q), negacyclic(a1[p], b0[p], q))]
        for k, d in enumerate((negacyclic(a0[p], b0[p], q), cross, negacyclic(a1[p], b1[p], q))):
            tensor[k].append([t * v % q for v in d])
    floor = [mod_down(d[L:], d[:L], Q, Bsk) for d in tensor]                                                                               # steps 5, 6
    if exact:
        out = [extend_exact(f[:K], f[K], B, Q, m_sk) for f in floor]                                                                       # step 7
    else:
        out = [extend_approx(f[:K], B, Q) for f in floor]
    return {"operands": operands, "tensor": tensor, "floor": floor, "out": out}
