// basis_coeff_kernels.hpp -- the coefficient-domain kernels of the basis calls: agx_ntt_basis_extend (basis_coeff_kernel), _extend_exact / _extend_mont
// (basis_aux_coeff_kernel), _quotient (basis_quotient_kernel) and the generic route of _mod_down / _mod_down_mode (moddown_coeff_kernel,
// moddown_coeff_round_kernel).  Compiled in ntt_kernels.hip.  One shape: one thread per (frame, coefficient), grid-stride over the batch x n coefficients, the
// words it keeps across the targets in registers under SMAX >= S, wave-uniform constants (scalar loads); dense layouts, no LDS, no barrier.
#pragma once
#include "ntt_kernels.hpp"
#include "modarith.hpp"
#include "moddown_arith.hpp"           // the two per-word steps of AGX_RESCALE_ROUND in moddown_coeff_round_kernel
#include "bfv_conv_arith.hpp"          // the per-word steps of agx_ntt_basis_extend_exact / _mont in basis_aux_coeff_kernel
#include "bfv_quotient_arith.hpp"      // those of agx_ntt_basis_quotient in basis_quotient_kernel

namespace agx {

// ---------------------------------------------------------------------------------------
// agx_ntt_basis_extend, coefficient form: fast RNS base conversion from S source primes to T target primes, dense layouts, out of place
// ---------------------------------------------------------------------------------------
// One thread per (frame, coefficient): it reads its S source words (slab i at x + i per_prime), forms every y_i = x_i D_i^-1 mod q_i once,
// then walks the T targets and writes one word each: 8 (S + T) bytes per coefficient, no source word read twice.  The constants are
// wave-uniform (scalar loads).  SMAX >= S bounds the y_i kept in registers (the loops over i are unrolled and guarded, never indexed).
template <int SMAX>
__global__ void basis_coeff_kernel(const uint64_t* __restrict__ x, uint64_t* __restrict__ out, const prime_consts* __restrict__ src_consts,
                                   const prime_consts* __restrict__ dst_consts, const ulonglong2* __restrict__ dinv, const ulonglong2* __restrict__ mat,
                                   uint32_t S, uint32_t T, uint64_t per_prime) {
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < per_prime; e += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t y[SMAX];
#pragma unroll
        for (int i = 0; i < SMAX; ++i)
            if ((uint32_t)i < S) {
                const ulonglong2 d = dinv[i];
                y[i] = basis_scale(x[(uint64_t)i * per_prime + e], d.x, d.y, src_consts[i].q);
            }
        for (uint32_t j = 0; j < T; ++j) {
            const uint64_t q = dst_consts[j].q, q2 = q << 1;
            const ulonglong2* row = mat + (size_t)j * S;
            uint64_t acc = 0;
#pragma unroll
            for (int i = 0; i < SMAX; ++i)
                if ((uint32_t)i < S) {
                    const ulonglong2 c = row[i];
                    acc = basis_accumulate(acc, y[i], c.x, c.y, q, q2);
                }
            out[(uint64_t)j * per_prime + e] = csub(acc, q);
        }
    }
}

// agx_ntt_basis_extend_exact (EXACT) and agx_ntt_basis_extend_mont, coefficient form: basis_coeff_kernel's shape -- one thread per (frame, coefficient),
// the y_i in registers under SMAX, wave-uniform constants -- with the correction by the auxiliary prime m (bfv_conv_arith.hpp).  A thread reads its S source
// words (and, EXACT, its word of the auxiliary slab), forms V mod m through one more constant row {D_i mod m} as it forms the y_i, then alpha ONCE (one
// Shoup product by k and the centring), and finishes every target with one Shoup product |alpha| c_j, added or subtracted by alpha's sign: 8 (S + 1 + T)
// bytes per coefficient (EXACT) or 8 (S + T).  The two forms differ in their constants alone (aux_set): the Montgomery form's m and m^-1 are folded into
// dinv, mat and c, and it reads no auxiliary word.
template <int SMAX, bool EXACT>
__global__ void basis_aux_coeff_kernel(const uint64_t* __restrict__ x, const uint64_t* __restrict__ xaux, uint64_t* __restrict__ out,
                                       const prime_consts* __restrict__ src_consts, const prime_consts* __restrict__ dst_consts, const ulonglong2* __restrict__ dinv,
                                       const ulonglong2* __restrict__ mat, const ulonglong2* __restrict__ row, const ulonglong2* __restrict__ corr, uint64_t m,
                                       uint64_t k, uint64_t kp, uint32_t S, uint32_t T, uint64_t per_prime) {
    const uint64_t m2 = m << 1;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < per_prime; e += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t y[SMAX];
        uint64_t vm = 0;
#pragma unroll
        for (int i = 0; i < SMAX; ++i)
            if ((uint32_t)i < S) {
                const ulonglong2 d = dinv[i], c = row[i];
                y[i] = basis_scale(x[(uint64_t)i * per_prime + e], d.x, d.y, src_consts[i].q);
                vm = basis_accumulate(vm, y[i], c.x, c.y, m, m2);
            }
        const uint64_t r = EXACT ? bfv_reduce_lazy(xaux[e], m) : 0;
        bool negative;
        const uint64_t mag = bfv_centre(bfv_alpha(csub(vm, m), r, k, kp, m), m, &negative);
        for (uint32_t j = 0; j < T; ++j) {
            const uint64_t q = dst_consts[j].q, q2 = q << 1;
            const ulonglong2* mrow = mat + (size_t)j * S;
            uint64_t acc = 0;
#pragma unroll
            for (int i = 0; i < SMAX; ++i)
                if ((uint32_t)i < S) {
                    const ulonglong2 c = mrow[i];
                    acc = basis_accumulate(acc, y[i], c.x, c.y, q, q2);
                }
            const ulonglong2 c = corr[j];
            out[(uint64_t)j * per_prime + e] = bfv_correct(acc, mag, negative, c.x, c.y, q);
        }
    }
}

// agx_ntt_basis_quotient, the coefficient-domain step: the fast floor on Bsk and the Shenoy-Kumaresan return to Q in one pass (bfv_quotient_arith.hpp has
// the formulas; S = K sources B, T = L targets Q, as the basis names them).  One thread per (frame, coefficient), basis_aux_coeff_kernel's shape: it reads
// the T words y_i that the scaled inverse of the Q slabs wrote (slab i at y + i per_prime) and adds each, as it arrives, into the S accumulators of the
// z_j and into f_m's through one row of qmat ([T][S + 1]) -- no y_i is kept -- then reads its S + 1 words s_j, s_m of the scaled inverse of the Bsk slabs
// (behind the y_i), finishes the z_j in [0, b_j) and f_m in [0, m), forms W mod m as it goes, alpha ONCE, and walks the T targets as the exact conversion
// does: 8 (2T + S + 1) bytes per coefficient and (2T + 1)(S + 1) Shoup products.  SMAX >= S bounds the z_j kept in registers (the loops over j are
// unrolled and guarded, never indexed); the loops over the T targets are not unrolled and keep nothing.  The constants are wave-uniform (scalar loads).
// No LDS, no barrier; out touches y nowhere.
template <int SMAX>
__global__ void basis_quotient_kernel(const uint64_t* __restrict__ y, uint64_t* __restrict__ out, const prime_consts* __restrict__ src_consts,
                                      const prime_consts* __restrict__ dst_consts, const ulonglong2* __restrict__ qmat, const ulonglong2* __restrict__ mat,
                                      const ulonglong2* __restrict__ row, const ulonglong2* __restrict__ corr, uint64_t m, uint64_t k, uint64_t kp, uint32_t S,
                                      uint32_t T, uint64_t per_prime) {
    const uint64_t m2 = m << 1;
    const uint64_t* __restrict__ sb = y + (uint64_t)T * per_prime;      // the S slabs s_j, then s_m's
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < per_prime; e += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t z[SMAX];
        uint64_t fm = 0;
#pragma unroll
        for (int j = 0; j < SMAX; ++j) z[j] = 0;
        for (uint32_t i = 0; i < T; ++i) {
            const uint64_t yi = y[(uint64_t)i * per_prime + e];
            const ulonglong2* qrow = qmat + (size_t)i * (S + 1);
#pragma unroll
            for (int j = 0; j < SMAX; ++j)
                if ((uint32_t)j < S) {
                    const ulonglong2 c = qrow[j];
                    const uint64_t b = src_consts[j].q;
                    z[j] = quot_accumulate(z[j], yi, c.x, c.y, b, b << 1);
                }
            const ulonglong2 c = qrow[S];
            fm = quot_accumulate(fm, yi, c.x, c.y, m, m2);
        }
        uint64_t wm = 0;
#pragma unroll
        for (int j = 0; j < SMAX; ++j)
            if ((uint32_t)j < S) {
                const ulonglong2 c = row[j];
                z[j] = quot_residue(sb[(uint64_t)j * per_prime + e], z[j], src_consts[j].q);
                wm = quot_accumulate(wm, z[j], c.x, c.y, m, m2);
            }
        fm = quot_residue(sb[(uint64_t)S * per_prime + e], fm, m);
        bool negative;
        const uint64_t mag = bfv_centre(bfv_alpha(csub(wm, m), fm, k, kp, m), m, &negative);
        for (uint32_t i = 0; i < T; ++i) {
            const uint64_t q = dst_consts[i].q, q2 = q << 1;
            const ulonglong2* mrow = mat + (size_t)i * S;
            uint64_t acc = 0;
#pragma unroll
            for (int j = 0; j < SMAX; ++j)
                if ((uint32_t)j < S) {
                    const ulonglong2 c = mrow[j];
                    acc = quot_accumulate(acc, z[j], c.x, c.y, q, q2);
                }
            const ulonglong2 c = corr[i];
            out[(uint64_t)i * per_prime + e] = bfv_correct(acc, mag, negative, c.x, c.y, q);
        }
    }
}

// agx_ntt_basis_mod_down, generic route, in the coefficient domain: out_j[e] <- (out_j[e] - sum_i y_i[e] (D_i mod q_j)) D^-1 mod q_j.  One thread
// per (frame, coefficient): it reads its S words of y (y_i in [0,q_i), as the scaled inverse of the source slabs wrote them: no basis_scale here),
// then reads, finishes and writes back one word of each of the T target slabs, which the inverse left in [0,q_j): 8 (S + 2T) bytes per
// coefficient.  The sum stays in [0,2q_j) term by term (basis_accumulate) and is brought below q_j for rescale_finish's reduced form, which
// never forms 4q: any modulus below 2^62.  Constants are wave-uniform.  SMAX >= S as in basis_coeff_kernel.
// AGX_RESCALE_ROUND (agx_ntt_basis_mod_down_mode) adds the two per-word steps of moddown_arith.hpp: c_i joins y_i modulo q_i as it is read, and
// t h mod q_j leaves the sum, which stays in [0,2q_j), before it is brought below q_j.  One body (moddown_coeff_body.hpp, included in both), two
// kernels: moddown_coeff_kernel (FLOOR: what it always was; rsrc and rdst are never read) and moddown_coeff_round_kernel.
template <int SMAX>
__global__ void moddown_coeff_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ y, const prime_consts* __restrict__ dst_consts,
                                     const ulonglong2* __restrict__ mat, const ulonglong2* __restrict__ dall, uint32_t S, uint32_t T, uint64_t per_prime) {
    [[maybe_unused]] constexpr bool ROUND = false;
    [[maybe_unused]] constexpr const ulonglong2* rsrc = nullptr;
    [[maybe_unused]] constexpr const uint64_t* rdst = nullptr;
#include "moddown_coeff_body.hpp"
}

// rsrc: [S] {c_i = h D_i^-1 mod q_i, q_i}; rdst: [T] t h mod q_j
template <int SMAX>
__global__ void moddown_coeff_round_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ y, const prime_consts* __restrict__ dst_consts,
                                           const ulonglong2* __restrict__ mat, const ulonglong2* __restrict__ dall, uint32_t S, uint32_t T, uint64_t per_prime,
                                           const ulonglong2* __restrict__ rsrc, const uint64_t* __restrict__ rdst) {
    [[maybe_unused]] constexpr bool ROUND = true;
#include "moddown_coeff_body.hpp"
}

}  // namespace agx
