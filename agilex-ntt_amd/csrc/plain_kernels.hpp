// plain_kernels.hpp -- the coefficient-domain kernels of agx_ntt_plain_scale_up / _lift (plain_encode_kernel) and of agx_ntt_plain_scale_down
// (plain_scale_down_kernel) and of agx_ntt_plain_reduce (plain_centred_reduce_kernel).  Compiled in ntt_kernels.hip.  The shape of basis_coeff_kernels.hpp: one thread per (frame, coefficient), grid-stride over the
// batch x n coefficients, wave-uniform constants (scalar loads); dense layouts, no LDS, no barrier.  plain_arith.hpp has the formulas and the ranges.
#pragma once
#include "ntt_kernels.hpp"
#include "plain_arith.hpp"

namespace agx {

// agx_ntt_plain_scale_up (LIFT = false) and agx_ntt_plain_lift (LIFT = true), coefficient form: m dense [batch][n], any 64-bit words -> out dense
// [L][batch][n], slab i under plan prime q_first + i (consts points at it), fully reduced.  A thread reads its word, reduces it modulo t, forms ONE signed
// value below t -- h - rho (scale_up: one product modulo t) or the centred m' (lift) -- and walks the L primes with one Shoup product each by cv.row[i]:
// {t^-1 mod q_i} or {1}.  8 (1 + L) bytes per coefficient.  out touches m nowhere.
template <bool LIFT>
__global__ void plain_encode_kernel(const uint64_t* __restrict__ m, uint64_t* __restrict__ out, const prime_consts* __restrict__ consts,
                                    const ulonglong2* __restrict__ row, uint64_t t, uint64_t h, uint64_t one_p, uint64_t d, uint64_t dp, uint32_t L,
                                    uint64_t per_prime) {
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < per_prime; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t mp = plain_reduce(m[e], one_p, t);
        bool negative;
        const uint64_t mag = LIFT ? plain_centred(mp, h, t, &negative) : plain_scaled(mp, d, dp, h, t, &negative);
        for (uint32_t i = 0; i < L; ++i) {
            const ulonglong2 c = row[i];
            out[(uint64_t)i * per_prime + e] = plain_residue(mag, negative, c.x, c.y, consts[i].q);
        }
    }
}

// agx_ntt_plain_scale_down, the coefficient-domain step: y dense [S][batch][n], y_i in [0, q_i) as the scaled inverse of the Q slabs wrote them (S = L), ->
// m dense [batch][n] in [0, t).  A thread reads its S words -- the loads of the unrolled, guarded loop under SMAX >= S are in flight together -- and adds each
// into the two sums through the rows {-q_i^-1 gamma^-1 mod t} and {-q_i^-1 mod gamma}, centres the gamma sum, applies ONE Shoup product by gamma^-1 mod t and
// stores one word: 8 (S + 1) bytes per coefficient and 2 S + 1 Shoup products.  m touches y nowhere.
template <int SMAX>
__global__ void plain_scale_down_kernel(const uint64_t* __restrict__ y, uint64_t* __restrict__ m, const ulonglong2* __restrict__ row_t,
                                        const ulonglong2* __restrict__ row_g, uint64_t t, uint64_t gamma, uint64_t g, uint64_t gp, uint32_t S,
                                        uint64_t per_prime) {
    const uint64_t t2 = t << 1, gamma2 = gamma << 1;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < per_prime; e += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t acc_t = 0, acc_g = 0;
#pragma unroll
        for (int i = 0; i < SMAX; ++i)
            if ((uint32_t)i < S) {
                const uint64_t yi = y[(uint64_t)i * per_prime + e];
                const ulonglong2 ct = row_t[i], cg = row_g[i];
                acc_t = quot_accumulate(acc_t, yi, ct.x, ct.y, t, t2);
                acc_g = quot_accumulate(acc_g, yi, cg.x, cg.y, gamma, gamma2);
            }
        m[e] = plain_round(acc_t, acc_g, gamma, g, gp, t);
    }
}

// agx_ntt_plain_reduce, the coefficient-domain step: y dense [S][batch][n], y_i in [0, q_i) as the plan's inverse of the Q slabs wrote them, -> m dense
// [batch][n] in [0, t): m = f X mod t for the centred X.  A thread reads its S words, forms the Garner digits and the sign as CKKS decode does
// (ckks_arith.hpp: S (S - 1) Shoup products), then S products modulo t through the row prod_{k < i} q_k mod t and one by f: 8 (S + 1) bytes per coefficient.
// m touches y nowhere.
template <int SMAX>
__global__ void plain_centred_reduce_kernel(const uint64_t* __restrict__ y, uint64_t* __restrict__ m, const uint64_t* __restrict__ q, const uint64_t* __restrict__ tri,
                                            const uint64_t* __restrict__ radix_t, uint64_t t, uint64_t d, uint64_t f, uint64_t fp, uint32_t S, uint64_t per_prime) {
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < per_prime; e += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t x[SMAX], v[SMAX];
#pragma unroll
        for (int i = 0; i < SMAX; ++i) x[i] = (uint32_t)i < S ? y[(uint64_t)i * per_prime + e] : 0;
        ckks_garner_digits<SMAX>(x, S, q, tri, v);
        m[e] = plain_from_digits<SMAX>(v, ckks_digits_negative<SMAX>(v, S, q), S, radix_t, t, d, f, fp);
    }
}

}  // namespace agx
