// ckks_arith.hpp -- the per-word steps of agx_ntt_ckks_encode and agx_ntt_ckks_decode (CKKS encoding and decoding: the special FFT over the rotation group
// in IEEE double, the rounding of a double into residues, and the exact RNS -> double conversion through mixed-radix digits), beside bfv_conv_arith.hpp, whose
// Shoup product it uses.  Compiles for the device (ckks_kernels.hpp) and for the host (tests/ckks_selftest.cpp runs this same text against unsigned __int128):
// no HIP header is needed on the host.  Every floating-point step is ONE IEEE operation: the build contracts nothing (-ffp-contract=off), so the numpy
// float64 model of tests/ckks_ref.py, which follows the same graph, gives the same bits.  include/agx_ntt.h has the definition.
//
//   ckks_mul          (a_r b_r - a_i b_i, a_r b_i + a_i b_r): four products, two sums.
//   ckks_bfly_fwd     decode's butterfly: w = b tw, (a, b) <- (a + w, a - w).
//   ckks_bfly_inv     encode's butterfly: (a, b) <- (a + b, (a - b) conj tw), conj tw = (tw_r, -tw_i).
//   ckks_round        any double x -> the integer c = rint(x), ties to even, as a sign and a magnitude mant 2^e: for |x| < 2^63, mant = |c| < 2^63 and e = 0;
//                     from 2^63 on x is an integer already, mant is its 53-bit significand and 11 <= e <= 971; a NaN or an infinity gives c = 0.
//   ckks_residue      c mod q in [0, q) from (negative, mant) and the pair {2^e mod q, its quotient}: one Shoup product (bfv_shoup), which takes ANY 64-bit mant and any
//                     q with 2q < 2^64 (bfv_conv_arith.hpp), and the sign; -0 = 0.
//   ckks_rns_to_double   the residues x_i in [0, q_i) of X modulo D = q_0 ... q_{L-1} -> the centred representative of X as a double:
//                     (1) the mixed-radix digits X mod D = v_0 + v_1 q_0 + v_2 q_0 q_1 + ..., v_i in [0, q_i):  t = x_i, then for j < i
//                         t = (t - v_j) q_j^-1 mod q_i, as t c - v_j c with c = q_j^-1 mod q_i (two Shoup products: v_j is a residue of another modulus);
//                     (2) the digits of (D - 1) / 2 are exactly (q_i - 1) / 2, so X mod D is above it -- X is negative -- iff the first digit from the top
//                         that differs from (q_i - 1) / 2 is greater;
//                     (3) the digits of D - 1 are q_i - 1, so |X| = D - (X mod D) has the digits q_i - 1 - v_i, plus 1 with a carry from the bottom;
//                     (4) Horner from the top in double, acc = acc (double)q_i + (double)w_i from acc = 0 (0 q + w = w exactly: the same bits as starting at
//                         (double)w_{L-1}); every conversion rounds to nearest even, every product and sum is one operation; (5) the sign.
//                     (1) and (2) are also functions of their own, ckks_garner_digits and ckks_digits_negative: plain_arith.hpp's plain_from_digits follows them.
//                     tri: the triangular table, the pair of q_j^-1 mod q_i at [i (i - 1) / 2 + j], two words each: a prefix serves a prefix of the primes.
#pragma once
#include "bfv_conv_arith.hpp"

namespace agx {

constexpr uint32_t kCkksPow2 = 1024;      // pairs of 2^e mod q_i per prime, e < 1024 (a finite double has e <= 971)

struct ckks_cplx {
    double re, im;
};

AGX_HD ckks_cplx ckks_mul(ckks_cplx a, ckks_cplx b) {
    const double rr = a.re * b.re, ii = a.im * b.im, ri = a.re * b.im, ir = a.im * b.re;
    return {rr - ii, ri + ir};
}

AGX_HD void ckks_bfly_fwd(ckks_cplx& a, ckks_cplx& b, ckks_cplx tw) {
    const ckks_cplx u = a, w = ckks_mul(b, tw);
    a = {u.re + w.re, u.im + w.im};
    b = {u.re - w.re, u.im - w.im};
}

AGX_HD void ckks_bfly_inv(ckks_cplx& a, ckks_cplx& b, ckks_cplx tw) {
    const ckks_cplx u = {a.re + b.re, a.im + b.im}, d = {a.re - b.re, a.im - b.im};
    a = u;
    b = ckks_mul(d, ckks_cplx{tw.re, -tw.im});
}

AGX_HD uint64_t ckks_round(double x, bool* negative, uint32_t* e) {
    uint64_t bits;
    __builtin_memcpy(&bits, &x, 8);
    const uint32_t ex = (uint32_t)(bits >> 52) & 0x7ffu;
    *negative = (bits >> 63) != 0;
    *e = 0;
    if (ex == 0x7ffu) return 0;                                                  // NaN, +-Inf
    if (ex < 1023u + 63u) return (uint64_t)__builtin_rint(__builtin_fabs(x));      // below 2^63: exact after the rounding
    *e = ex - 1075u;
    return (bits & ((1ull << 52) - 1)) | (1ull << 52);
}

AGX_HD uint64_t ckks_residue(uint64_t mant, bool negative, uint64_t w, uint64_t wp, uint64_t q) {
    const uint64_t p = bfv_shoup(mant, w, wp, q);      // |c| mod q in [0, q)
    return negative && p ? q - p : p;                   // -0 = 0
}

// steps (1) and (2) of ckks_rns_to_double on their own: agx_ntt_plain_reduce (plain_arith.hpp) takes the same digits and the same sign to a residue modulo t
template <int SMAX>
AGX_HD void ckks_garner_digits(const uint64_t (&x)[SMAX], uint32_t L, const uint64_t* q, const uint64_t* tri, uint64_t (&v)[SMAX]) {
#pragma unroll
    for (int i = 0; i < SMAX; ++i) {
        v[i] = 0;
        if ((uint32_t)i < L) {
            const uint64_t qi = q[i];
            uint64_t t = x[i];
#pragma unroll
            for (int j = 0; j < i; ++j) {
                const uint64_t c = tri[2 * (i * (i - 1) / 2 + j)], cp = tri[2 * (i * (i - 1) / 2 + j) + 1];
                const uint64_t a = bfv_shoup(t, c, cp, qi), b = bfv_shoup(v[j], c, cp, qi);
                t = a - b + (a < b ? qi : 0);
            }
            v[i] = t;
        }
    }
}

template <int SMAX>
AGX_HD bool ckks_digits_negative(const uint64_t (&v)[SMAX], uint32_t L, const uint64_t* q) {
    bool negative = false, decided = false;
#pragma unroll
    for (int i = SMAX - 1; i >= 0; --i)
        if ((uint32_t)i < L && !decided && v[i] != (q[i] >> 1)) negative = v[i] > (q[i] >> 1), decided = true;
    return negative;
}

// ckks_rns_to_double keeps steps (1) and (2) in its own body, the same statements as the two functions above: calling them here changed the code the compiler
// generates for every ckks_decode_kernel instance (tools/compare_device_asm.py), and those kernels stay as they were measured.
template <int SMAX>
AGX_HD double ckks_rns_to_double(const uint64_t (&x)[SMAX], uint32_t L, const uint64_t* q, const uint64_t* tri) {
    uint64_t v[SMAX];
#pragma unroll
    for (int i = 0; i < SMAX; ++i) {
        v[i] = 0;
        if ((uint32_t)i < L) {
            const uint64_t qi = q[i];
            uint64_t t = x[i];
#pragma unroll
            for (int j = 0; j < i; ++j) {
                const uint64_t c = tri[2 * (i * (i - 1) / 2 + j)], cp = tri[2 * (i * (i - 1) / 2 + j) + 1];
                const uint64_t a = bfv_shoup(t, c, cp, qi), b = bfv_shoup(v[j], c, cp, qi);
                t = a - b + (a < b ? qi : 0);
            }
            v[i] = t;
        }
    }
    bool negative = false, decided = false;
#pragma unroll
    for (int i = SMAX - 1; i >= 0; --i)
        if ((uint32_t)i < L && !decided && v[i] != (q[i] >> 1)) negative = v[i] > (q[i] >> 1), decided = true;
    bool carry = negative;
#pragma unroll
    for (int i = 0; i < SMAX; ++i)
        if ((uint32_t)i < L && negative) {
            uint64_t w = q[i] - 1 - v[i];
            if (carry) {
                ++w;
                if (w == q[i]) w = 0;
                else carry = false;
            }
            v[i] = w;
        }
    double acc = 0.0;
#pragma unroll
    for (int i = SMAX - 1; i >= 0; --i)
        if ((uint32_t)i < L) {
            const double p = acc * (double)q[i];
            acc = p + (double)v[i];
        }
    return negative ? -acc : acc;
}

}  // namespace agx
