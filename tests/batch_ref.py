"""The Python-integer reference model of agx_ntt_batch_encode / _decode (SIMD batching of BFV / BGV) and of agx_ntt_plain_reduce (BGV decryption: the exact
centred conversion Q -> t); include/agx_ntt.h has the contract.  Python integers and nothing else.  The GPU tests are judged against this module; this module
is judged on the CPU by tests/test_batch_reference.py.

Batching: M = 2n, t prime with t = 1 (mod M), psi the least primitive M-th root of unity modulo t, e_j = 5^j mod M for j < n / 2 and e_{n/2+j} = M - e_j;
decode is z_j = m(psi^{e_j}) mod t, encode its inverse.  A frame is a list [n]."""
import functools


def is_prime(q):
    if q < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if q % p == 0:
            return q == p
    d, s = q - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):      # decides every 64-bit number
        y = pow(a, d, q)
        if y in (1, q - 1):
            continue
        for _ in range(s - 1):
            y = y * y % q
            if y == q - 1:
                break
        else:
            return False
    return True


@functools.lru_cache(maxsize=None)
def min_root(t, n):
    """the least primitive 2n-th root of unity modulo the prime t = 1 (mod 2n): what agx_ntt_min_root returns"""
    M = 2 * n
    assert is_prime(t) and (t - 1) % M == 0
    g = next(r for r in (pow(a, (t - 1) // M, t) for a in range(2, t)) if pow(r, n, t) == t - 1)
    least, walk, sq = g, g, g * g % t
    for _ in range(n - 1):      # the primitive roots are the odd powers of any one of them
        walk = walk * sq % t
        least = min(least, walk)
    return least


@functools.lru_cache(maxsize=None)
def exponents(n):
    """(e_0, ..., e_{n-1})"""
    M, row, e = 2 * n, [], 1
    for _ in range(max(n // 2, 1)):
        row.append(e)
        e = e * 5 % M
    return tuple(row + [M - v for v in row])


def brev(k, bits):
    r = 0
    for _ in range(bits):
        r, k = (r << 1) | (k & 1), k >> 1
    return r


@functools.lru_cache(maxsize=None)
def slot_to_word(n):
    """pos(j) = brev((e_j - 1) / 2) over log2 n bits: where slot j sits in the library's NTT order out[brev(k)] = x(psi^{2k+1})"""
    bits = n.bit_length() - 1
    return tuple(brev((e - 1) // 2, bits) for e in exponents(n))


def evaluate(m, x, t):
    """m(x) mod t by Horner"""
    acc = 0
    for c in reversed(m):
        acc = (acc * x + int(c)) % t
    return acc


def decode_slot(m, n, t, j):
    """z_j = m(psi^{e_j}) mod t: one slot, the definition itself"""
    return evaluate(m, pow(min_root(t, n), exponents(n)[j], t), t)


def decode(m, n, t):
    """m [n] in [0, t) -> z [n]: every slot by the definition (O(n^2): small n)"""
    return [decode_slot(m, n, t, j) for j in range(n)]


def _ntt_natural(m, n, t):
    """[m(psi^{2k+1}) for k < n] by a recursive negacyclic transform in Python integers, O(n log n)"""
    psi = min_root(t, n)
    a = [int(c) % t * pow(psi, i, t) % t for i, c in enumerate(m)]      # twist: m(psi w^k) = sum (m_i psi^i) w^{ik}, w = psi^2

    def fft(v, w):
        if len(v) == 1:
            return v
        even, odd = fft(v[0::2], w * w % t), fft(v[1::2], w * w % t)
        out, x, half = [0] * len(v), 1, len(v) // 2
        for k in range(half):
            u = x * odd[k] % t
            out[k], out[k + half] = (even[k] + u) % t, (even[k] - u) % t
            x = x * w % t
        return out

    return fft(a, psi * psi % t)


def decode_fast(m, n, t):
    """decode by the O(n log n) transform: z_j = m(psi^{2k+1}) with 2k + 1 = e_j"""
    nat = _ntt_natural(m, n, t)
    return [nat[(e - 1) // 2] for e in exponents(n)]


def encode(z, n, t):
    """z [n], any integers (taken modulo t) -> m [n] in [0, t) with decode(m) = z mod t: m_i = n^-1 sum_j z_j psi^{-e_j i}, through the same transform run
    on the conjugate root: sum_j z_j (psi^-1)^{e_j i}"""
    psi_inv = pow(min_root(t, n), -1, t)
    # m_i = n^-1 Z(psi^-i) with Z(y) = sum_j z_j y^{e_j}: a polynomial of degree < 2n with the odd coefficients z at e_j
    by_exp = [0] * (2 * n)
    for zj, e in zip(z, exponents(n)):
        by_exp[e] = int(zj) % t
    # Z(psi^-i) = sum_k by_exp[2k+1] psi^-(2k+1)i: fold the odd part into a length-n sum with w = psi^-2
    odd = [by_exp[2 * k + 1] for k in range(n)]
    n_inv = pow(n, -1, t)
    if n <= 64:
        return [n_inv * pow(psi_inv, i, t) * sum(c * pow(psi_inv, 2 * k * i, t) for k, c in enumerate(odd)) % t for i in range(n)]

    def fft(v, w):
        if len(v) == 1:
            return v
        even, o = fft(v[0::2], w * w % t), fft(v[1::2], w * w % t)
        out, x, half = [0] * len(v), 1, len(v) // 2
        for k in range(half):
            u = x * o[k] % t
            out[k], out[k + half] = (even[k] + u) % t, (even[k] - u) % t
            x = x * w % t
        return out

    spectrum = fft(odd, psi_inv * psi_inv % t)      # spectrum[i] = sum_k odd[k] psi^{-2ki}
    return [n_inv * pow(psi_inv, i, t) * spectrum[i] % t for i in range(n)]


def negacyclic(a, b, t):
    """a b mod (X^n + 1, t), schoolbook"""
    n, out = len(a), [0] * len(a)
    for i, u in enumerate(a):
        for j, v in enumerate(b):
            k = i + j
            if k < n:
                out[k] = (out[k] + u * v) % t
            else:
                out[k - n] = (out[k - n] - u * v) % t
    return out


def automorphism(m, g, t):
    """sigma_g: X -> X^g on coefficients, modulo (X^n + 1, t)"""
    n, out = len(m), [0] * len(m)
    for i, c in enumerate(m):
        k = i * g % (2 * n)
        if k < n:
            out[k] = int(c) % t
        else:
            out[k - n] = -int(c) % t
    return out


def rotate_rows(z, r):
    """both rows of z [n] rotated left by r"""
    h = len(z) // 2
    return [z[(j + r) % h] for j in range(h)] + [z[h + (j + r) % h] for j in range(h)]


def swap_rows(z):
    h = len(z) // 2
    return list(z[h:]) + list(z[:h])


# ---- agx_ntt_plain_reduce ----

def product(Q):
    D = 1
    for q in Q:
        D *= q
    return D


def centred_value(residues, Q):
    """the integer X in [-(D - 1) / 2, (D - 1) / 2] with X = residues[i] (mod Q[i]): CRT in Python integers"""
    D, X = product(Q), 0
    for r, q in zip(residues, Q):
        Qi = D // q
        X = (X + int(r) % q * pow(Qi, -1, q) * Qi) % D
    return X - D if X > (D - 1) // 2 else X


def reduce(x, Q, t, factor=1):
    """x [L][count] coefficient-form words (any words) -> [count] in [0, t): (factor mod t) X mod t for the centred X; no inverse modulo t anywhere"""
    return [(factor % t) * centred_value([xi[e] for xi in x], Q) % t for e in range(len(x[0]))]


def reduce_device_form(x, Q, t, factor=1):
    """the same words as the device forms them: Garner digits, the sign against the digits of (D - 1) / 2, sum v_i (prod_{k<i} q_k mod t) - [neg] (D mod t)"""
    out = []
    for e in range(len(x[0])):
        v = []
        for i, q in enumerate(Q):
            w = int(x[i][e]) % q
            for j in range(i):
                w = (w - v[j]) * pow(Q[j], -1, q) % q
            v.append(w)
        negative = False
        for vi, q in zip(reversed(v), reversed(Q)):
            if vi != q >> 1:
                negative = vi > q >> 1
                break
        acc, weight = 0, 1
        for vi, q in zip(v, Q):
            acc = (acc + vi * (weight % t)) % t
            weight *= q
        if negative:
            acc = (acc - weight % t) % t
        out.append(acc * (factor % t) % t)
    return out
