// inner_reduce.hpp -- the accumulate-and-reduce step of agx_ntt_inner_product: sum_t a_t b_t kept in 128 bits, reduced modulo q once.
// Compiles for the device (inner_product_kernel, inner_kernels.hpp) and for the host (tests/inner_selftest.cpp runs this same text against
// unsigned __int128 %): no HIP header is needed on the host, the high product is portable there.
//
// Range argument.
//   Terms.  Operands are reduced to [0, q) first and q < 2^62, so a product is below 2^124 and sixteen of them stay below 2^128: the sum of up
//   to AGX_INNER_MAX_TERMS = 16 products never wraps its {hi, lo} pair (the same count as AGX_BASIS_MAX_SRC, for the same reason).
//   Reduction.  Let x = hi 2^64 + lo be ANY 128-bit value, mu = mu_hi 2^64 + mu_lo = floor(2^128 / q), so 2^128 / q - 1 < mu <= 2^128 / q.
//   Then x mu / 2^128 lies in (x / q - x / 2^128, x / q] and x / 2^128 < 1: e_full = floor(x mu / 2^128) is floor(x / q) or one less.
//     x mu = hi mu_hi 2^128 + (hi mu_lo + lo mu_hi) 2^64 + lo mu_lo.
//   The estimate est = hi mu_hi + umulhi(hi, mu_lo) + umulhi(lo, mu_hi) leaves out the low halves of the two cross products (each below 2^64,
//   together below 2 2^64: at most 2 2^128 of x mu) and lo mu_lo (below 2^128): less than 3 2^128 in all, so e_full - est <= 2 and
//   floor(x / q) - est <= 3.  The remainder r = x - est q therefore lies in [0, 4q), and 4q < 2^64 because q < 2^62: r is represented exactly
//   by its low word, lo - est q mod 2^64, whatever est and hi mu_hi do modulo 2^64 (for a small q the quotient itself does not fit a word;
//   only the difference matters).  Two conditional subtracts (2q, then q) finish.  This is the tail of mul_mod_barrett (modarith.hpp) fed with
//   a sum instead of one product.  tests/inner_selftest.cpp: 1, 2, 15 and 16 terms of (q - 1)^2, random sums, random 128-bit values, moduli of
//   2, 17, 30, 31, 60, 61 and 62 bits; the largest multiple of q it finds before the subtracts is reported there.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AGX_HD __host__ __device__ __forceinline__
#else
#define AGX_HD inline
#endif

namespace agx {

AGX_HD uint64_t umulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

struct acc128 {
    uint64_t lo = 0, hi = 0;
};

// s += a b; a, b < q < 2^62, at most sixteen times per sum (see above)
AGX_HD void acc_mul_add(acc128& s, uint64_t a, uint64_t b) {
    const uint64_t lo = a * b, hi = umulhi64(a, b);
    s.lo += lo;
    s.hi += hi + (s.lo < lo ? 1u : 0u);
}

// x - est q before the conditional subtracts: in [0, 4q) for ANY 128-bit x and any odd q < 2^62 with {mu_hi, mu_lo} = floor(2^128 / q)
AGX_HD uint64_t acc_reduce_lazy(const acc128& x, uint64_t q, uint64_t mu_hi, uint64_t mu_lo) {
    const uint64_t est = x.hi * mu_hi + umulhi64(x.hi, mu_lo) + umulhi64(x.lo, mu_hi);
    return x.lo - est * q;
}

// x mod q in [0, q)
AGX_HD uint64_t acc_reduce(const acc128& x, uint64_t q, uint64_t mu_hi, uint64_t mu_lo) {
    uint64_t r = acc_reduce_lazy(x, q, mu_hi, mu_lo);
    const uint64_t q2 = q << 1;
    r = r >= q2 ? r - q2 : r;
    return r >= q ? r - q : r;
}

}  // namespace agx
