"""The reference model of agx_ntt_ckks_encode and agx_ntt_ckks_decode (include/agx_ntt.h has the definition): the fixed operation graph in numpy float64, one
vectorised step per stage and one IEEE operation per numpy call (real and imaginary parts are kept apart, so no complex product of numpy's is used), Python
integers for Garner and the residues, the twiddles read through agx_ntt_ckks_twiddle.  The device is compared with this module bit for bit
(tests/test_gpu_ckks.py); this module is judged on the CPU by tests/test_ckks_reference.py against exact_*: the closed forms in high precision, mpmath at 200
bits where it imports, numpy.longdouble with pairwise sums otherwise.

A slot vector is a complex128 array [batch][s]; a frame set is a uint64 array [L][batch][n], slab i under Q[i]."""
import functools
import math

import numpy as np

try:
    import mpmath
except ImportError:      # the fallback below serves
    mpmath = None

U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def twiddle_table(half):
    """(re, im) float64 arrays [half]: tw(len, j) at len / 2 + j for len = 2 ... half; entry 0 is never read"""
    import agilex_ntt_amd as agx

    re, im = np.ones(max(half, 1)), np.zeros(max(half, 1))
    length = 2
    while length <= half:
        for j in range(length // 2):
            re[length // 2 + j], im[length // 2 + j] = agx.ckks_twiddle(length, j)
        length *= 2
    return re, im


@functools.lru_cache(maxsize=None)
def bitrev(s):
    bits = s.bit_length() - 1
    return np.array([int(format(k, f"0{bits}b")[::-1], 2) if bits else 0 for k in range(s)], dtype=np.int64)


def fft_forward(re, im):
    """decode's core on [batch][s]: bit-reverse, then len = 2, 4, ..., s"""
    s = re.shape[-1]
    tr, ti = twiddle_table(max(s, 2))
    re, im = re[..., bitrev(s)].copy(), im[..., bitrev(s)].copy()
    length = 2
    while length <= s:
        h = length // 2
        r, i = re.reshape(-1, s // length, length), im.reshape(-1, s // length, length)
        wr, wi = tr[h:length], ti[h:length]
        ar, ai, br, bi = r[..., :h].copy(), i[..., :h].copy(), r[..., h:].copy(), i[..., h:].copy()
        pr = br * wr - bi * wi
        pi = br * wi + bi * wr
        r[..., :h], i[..., :h] = ar + pr, ai + pi
        r[..., h:], i[..., h:] = ar - pr, ai - pi
        length *= 2
    return re, im


def fft_inverse(re, im):
    """encode's core on [batch][s]: len = s, s / 2, ..., 2, then bit-reverse (the 1 / s is the caller's)"""
    s = re.shape[-1]
    tr, ti = twiddle_table(max(s, 2))
    re, im = re.copy(), im.copy()
    length = s
    while length >= 2:
        h = length // 2
        r, i = re.reshape(-1, s // length, length), im.reshape(-1, s // length, length)
        wr, wi = tr[h:length], -ti[h:length]
        ar, ai, br, bi = r[..., :h].copy(), i[..., :h].copy(), r[..., h:].copy(), i[..., h:].copy()
        dr, di = ar - br, ai - bi
        r[..., :h], i[..., :h] = ar + br, ai + bi
        r[..., h:] = dr * wr - di * wi
        i[..., h:] = dr * wi + di * wr
        length //= 2
    return re[..., bitrev(s)], im[..., bitrev(s)]


def round_to_int(x):
    """c = rint(x), ties to even, as a Python integer; a NaN or an infinity gives 0"""
    return int(np.rint(x)) if math.isfinite(x) else 0


def encode_integers(z, n, scale):
    """z complex128 [batch][s] -> the integers c [batch][n] (Python integers, nested lists)"""
    z = np.asarray(z, dtype=np.complex128)
    batch, s = z.shape
    gap = (n // 2) // s
    with np.errstate(all="ignore"):
        re, im = fft_inverse(z.real.copy(), z.imag.copy())
        inv_s = 1.0 / s
        xr, xi = scale * (re * inv_s), scale * (im * inv_s)
    out = []
    for f in range(batch):
        row = [0] * n
        for k, (a, b) in enumerate(zip(xr[f].tolist(), xi[f].tolist())):
            row[k * gap], row[(k + s) * gap] = round_to_int(a), round_to_int(b)
        out.append(row)
    return out


def encode(z, n, Q, scale):
    """z complex128 [batch][s] -> uint64 [L][batch][n] in coefficient form"""
    c = encode_integers(z, n, scale)
    return np.array([[[v % q for v in row] for row in c] for q in Q], dtype=np.uint64)


def garner_digits(x, Q):
    """the residues x[i] in [0, Q[i]) -> the mixed-radix digits v: X mod D = v_0 + v_1 Q_0 + v_2 Q_0 Q_1 + ..."""
    v = []
    for i, q in enumerate(Q):
        t = int(x[i])
        for j in range(i):
            t = (t - v[j]) * pow(Q[j], -1, q) % q
        v.append(t)
    return v


def centred_digits(v, Q):
    """(negative, magnitude digits): the comparison from the top with (q_i - 1) / 2, the complement q_i - 1 - v_i plus 1 with a carry from the bottom"""
    negative = False
    for vi, q in zip(reversed(v), reversed(Q)):
        if vi != q >> 1:
            negative = vi > q >> 1
            break
    if not negative:
        return False, list(v)
    w, carry = [], True
    for vi, q in zip(v, Q):
        d = q - 1 - vi
        if carry:
            d += 1
            if d == q:
                d = 0
            else:
                carry = False
        w.append(d)
    return True, w


def rns_to_double(x, Q):
    """the residues of X -> the centred representative as the float the definition's Horner gives"""
    negative, w = centred_digits(garner_digits(x, Q), Q)
    acc = float(w[-1])
    for d, q in zip(reversed(w[:-1]), reversed(Q[:-1])):
        acc = acc * float(q) + float(d)
    return -acc if negative else acc


def decode(x, n, Q, scale, s):
    """x [L][batch][n] fully reduced words -> complex128 [batch][s]"""
    x = np.asarray(x)
    batch = x.shape[1]
    gap = (n // 2) // s
    cols = x[:, :, ::gap].astype(object)      # [L][batch][2s] Python integers
    vals = np.array([[rns_to_double([cols[i][f][k] for i in range(len(Q))], Q) for k in range(2 * s)] for f in range(batch)], dtype=np.float64).reshape(batch, 2 * s)
    re, im = fft_forward(vals[:, :s].copy(), vals[:, s:].copy())
    inv = 1.0 / scale
    return (re * inv) + 1j * (im * inv)


def centred(x, Q):
    """the residues [L][count] -> the centred integers [count] (CRT in Python integers)"""
    D = math.prod(Q)
    X = [0] * len(x[0])
    for xi, q in zip(x, Q):
        m = D // q
        c = m * pow(m, -1, q)
        X = [(a + int(b) * c) % D for a, b in zip(X, xi)]
    return [a - D if a > D // 2 else a for a in X]


# ---- exact_*: the closed forms in high precision ----

PRECISION_BITS = 200


def _in_precision(f):
    @functools.wraps(f)
    def g(*a, **k):
        if mpmath is None:
            return f(*a, **k)
        with mpmath.workprec(PRECISION_BITS):
            return f(*a, **k)
    return g


@functools.lru_cache(maxsize=4)
def _roots(s):
    """zeta'^m for m < 4s, zeta' = exp(i pi / (2s)): mpmath at 200 bits by repeated products from the exactly reduced first root (the error, 4s steps of
    2^-200, is far below every tolerance), or longdouble pairs from an exact integer octant reduction"""
    if mpmath is not None:
        with mpmath.workprec(PRECISION_BITS):
            first = mpmath.mpc(mpmath.cospi(mpmath.mpf(1) / (2 * s)), mpmath.sinpi(mpmath.mpf(1) / (2 * s)))
            r = [mpmath.mpc(1)]
            for _ in range(4 * s - 1):
                r.append(r[-1] * first)
            return r
    assert np.finfo(np.longdouble).nmant >= 63
    m = np.arange(4 * s)
    quadrant, rest = m // s, m % s
    swap = rest > s // 2
    rr = np.where(swap, s - rest, rest).astype(np.longdouble)
    phi = (np.longdouble(8) * np.arctan(np.longdouble(1)) * rr) / np.longdouble(4 * s)      # 2 pi rr / (4s) in [0, pi / 4]
    c, sn = np.cos(phi), np.sin(phi)
    c, sn = np.where(swap, sn, c), np.where(swap, c, sn)
    re = np.select([quadrant == 0, quadrant == 1, quadrant == 2], [c, -sn, -c], sn)
    im = np.select([quadrant == 0, quadrant == 1, quadrant == 2], [sn, c, -sn], -c)
    return re, im


def root(s, m):
    """(re, im) of zeta'^m, zeta' = exp(i pi / (2s)), as high-precision reals"""
    r = _roots(s)
    return (r[m % (4 * s)].real, r[m % (4 * s)].imag) if mpmath is not None else (r[0][m % (4 * s)], r[1][m % (4 * s)])


def _pairwise(values):
    values = list(values)
    while len(values) > 1:
        values = [values[i] + values[i + 1] if i + 1 < len(values) else values[i] for i in range(0, len(values), 2)]
    return values[0]


def _dot(weights, exps, s):
    """sum_i weights[i] zeta'^exps[i]: weights real or complex numbers (Python integers, floats, complex), the exponents reduced modulo 4s"""
    r = _roots(s)
    if mpmath is not None:
        with mpmath.workprec(PRECISION_BITS):
            acc = mpmath.mpc(0)
            for w, e in zip(weights, exps):
                w = mpmath.mpc(w.real, w.imag) if isinstance(w, complex) else mpmath.mpf(w)
                acc += w * r[e % (4 * s)]
            return acc
    re, im = r
    terms = []
    for w, e in zip(weights, exps):
        wr, wi = (np.longdouble(w.real), np.longdouble(w.imag)) if isinstance(w, complex) else (np.longdouble(w), np.longdouble(0))
        a, b = re[e % (4 * s)], im[e % (4 * s)]
        terms.append((wr * a - wi * b, wr * b + wi * a))
    return HpComplex(_pairwise([t[0] for t in terms]), _pairwise([t[1] for t in terms]))


@_in_precision
def exact_decode(X, n, s, scale, js):
    """X: the centred integer coefficients [n] -> {j: z_j} for the sampled slots js, as (re, im) floats holding the exact values to double precision and as
    high-precision numbers: returns {j: high-precision complex}"""
    gap = (n // 2) // s
    grid = [int(X[k * gap]) for k in range(2 * s)]
    out = {}
    for j in js:
        g = pow(5, j, 4 * s)
        out[j] = _dot(grid, [g * k for k in range(2 * s)], s) / _hp(scale)
    return out


@_in_precision
def exact_encode(z, s, ks):
    """z: complex slots [s] -> {k: w_k} for the sampled k < s, w_k = (1 / s) sum_j z_j zeta'^(-5^j k), in high precision (the scale is the caller's)"""
    gs = [pow(5, j, 4 * s) for j in range(s)]
    zs = [complex(v) for v in z]
    return {k: _dot(zs, [-g * k for g in gs], s) / s for k in ks}


class HpComplex:
    """the fallback's complex number: two longdoubles"""

    def __init__(self, real, imag):
        self.real, self.imag = real, imag

    def __truediv__(self, d):
        return HpComplex(self.real / np.longdouble(d), self.imag / np.longdouble(d))


def _hp(v):
    if mpmath is not None:
        return mpmath.mpf(v)
    return np.longdouble(v)


@_in_precision
def distance(value, exact):
    """|value - exact| as a float: value a float or a Python integer, exact a high-precision real"""
    return float(abs(_hp(value) - exact))


@_in_precision
def scaled(scale, exact):
    """scale * exact in high precision"""
    return _hp(scale) * exact


@_in_precision
def nearest_and_margin(exact):
    """(the integer nearest to a high-precision real, its distance from the nearest half-integer as a float)"""
    if mpmath is not None:
        lo = mpmath.floor(exact)
        frac = exact - lo
        return int(lo) + (1 if frac > mpmath.mpf(1) / 2 else 0), float(abs(frac - mpmath.mpf(1) / 2))
    lo = np.floor(exact)
    frac = exact - lo
    return int(lo) + (1 if frac > 0.5 else 0), float(abs(frac - np.longdouble(0.5)))
