// weighted_kernels.hpp -- the kernels of agx_ntt_keyswitch_accumulate_decomposed and agx_ntt_mul_add_galois: a linear transform's sum over rotations,
// formed in the extended basis before ONE ModDown (include/agx_ntt.h).  Compiled in ntt_kernels.hip.  inner_args, inner_lanes, inner_gather and
// galois_read_index of inner_kernels.hpp and ring_args of ring_kernels.hpp serve here as they stand.  The per-word finish is csrc/weighted_arith.hpp,
// which tests/weighted_selftest.cpp compiles too.
//
// Both have the streaming shape of inner_product_kernel: blockIdx.y is the slot of a prime, grid-stride over the slot's batch x n words; no LDS, no
// barrier, no table; W is one word, or a 16-byte pair when ALL bases of the call are 16-byte aligned.  pi_g is formed once per work item; GALOIS =
// false is the un-gathered kernel the host sends g = 1 to.  The output (acc, c) is read, when the call accumulates, and written by the same work item at
// the same index, so it carries no __restrict__; the host rules keep it apart from every other operand (c may be exactly b at g = 1: a work item then
// reads its own word of b before it writes it).  has_weight, accumulate and the broadcasts are wave-uniform.
#pragma once
#include "inner_kernels.hpp"
#include "ring_kernels.hpp"
#include "weighted_arith.hpp"

namespace agx {

__device__ __forceinline__ uint64_t weighted_lanes(const acc128* s, bool has_w, uint64_t w, bool has_old, uint64_t old, const prime_consts& k, uint64_t q2) {
    return weighted_finish(acc_reduce(s[0], k.q, k.mu_hi, k.mu_lo), has_w, w, has_old, old, k.q, q2, k.mu_hi, k.mu_lo);
}
__device__ __forceinline__ ulonglong2 weighted_lanes(const acc128* s, bool has_w, ulonglong2 w, bool has_old, ulonglong2 old, const prime_consts& k, uint64_t q2) {
    return make_ulonglong2(weighted_finish(acc_reduce(s[0], k.q, k.mu_hi, k.mu_lo), has_w, w.x, has_old, old.x, k.q, q2, k.mu_hi, k.mu_lo),
                           weighted_finish(acc_reduce(s[1], k.q, k.mu_hi, k.mu_lo), has_w, w.y, has_old, old.y, k.q, q2, k.mu_hi, k.mu_lo));
}

// acc_o[i] = (accumulate ? acc_o[i]' : 0) + w[i or its position in the frame]' (sum_t a_t[pi_g(i)]' key_{t,o}[i]') for o = 0, 1: inner_product_kernel's
// sum with two outputs, its groups of four terms and its 128-bit sums, then weighted_finish per word.  The weight's and the old words' loads are issued in
// front of the terms', so that they are in flight with them: 2 + 2 W more per work item than the plain kernel holds beside a group's 12.
struct weighted_args {
    inner_args in;
    uint64_t w_prime;                        // weight stride per slot in W: weight_batch n / lanes
    uint32_t log_n, g;                       // g odd, below 2n (GALOIS only)
    uint32_t has_weight, w_broadcast, accumulate;      // w_broadcast: the weight index is the key's (the position within the frame)
};

template <bool GALOIS, class W>
__global__ void inner_weighted_kernel(const W* __restrict__ a, const W* __restrict__ bhat, const W* __restrict__ wt, W* acc, const prime_consts* __restrict__ consts,
                                      weighted_args ga) {
    constexpr int kLanes = sizeof(W) / 8, kGroup = 4, OUT = 2;
    const inner_args& g = ga.in;
    const uint32_t slot = blockIdx.y;
    const prime_consts k = consts[slot < g.split ? slot : slot + g.skip];
    const uint64_t q2 = k.q << 1;
    const W* ap = a + (uint64_t)slot * g.per_prime;
    const W* bp = bhat + (uint64_t)slot * g.b_prime;
    const W* wp = wt + (uint64_t)slot * ga.w_prime;
    W* cp = acc + (uint64_t)slot * g.per_prime;
    const bool has_w = ga.has_weight != 0, has_old = ga.accumulate != 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.per_prime; i += (uint64_t)gridDim.x * blockDim.x) {
        bool swap = false;
        uint64_t ai = i;
        if constexpr (GALOIS) ai = galois_read_index<kLanes>(i, g.frame_mask, ga.log_n, ga.g, swap);
        const uint64_t fi = i & g.frame_mask, bi = g.broadcast ? fi : i;
        W w{}, old[OUT]{};
        if (has_w) w = wp[ga.w_broadcast ? fi : i];
        if (has_old) {
#pragma unroll
            for (int o = 0; o < OUT; ++o) old[o] = cp[o * g.c_out + i];
        }
        acc128 s[OUT][kLanes];
        for (uint32_t t0 = 0; t0 < g.terms; t0 += kGroup) {
            W av[kGroup], bv[kGroup][OUT];
#pragma unroll
            for (int u = 0; u < kGroup; ++u)
                if (t0 + u < g.terms) {
                    av[u] = ap[(t0 + u) * g.a_term + ai];
#pragma unroll
                    for (int o = 0; o < OUT; ++o) bv[u][o] = bp[(t0 + u) * g.b_term + o * g.b_out + bi];
                }
#pragma unroll
            for (int u = 0; u < kGroup; ++u)
                if (t0 + u < g.terms) {
#pragma unroll
                    for (int o = 0; o < OUT; ++o) inner_lanes(s[o], inner_gather(av[u], swap), bv[u][o], k.q, q2);
                }
        }
#pragma unroll
        for (int o = 0; o < OUT; ++o) cp[o * g.c_out + i] = weighted_lanes(s[o], has_w, w, has_old, old[o], k, q2);
    }
}

// agx_ntt_mul_add_galois: c[i] = (accumulate ? c[i]' : 0) + w[i or its position in the frame]' b[pi_g(i)]' on the plan primes [first, first + count): the
// gathered add's shape (ring_linear_kernel, GALOIS) with a product.  32 bytes per word with a weight per frame and an old word, 16 with neither.
struct mul_add_args {
    ring_args in;
    uint64_t w_prime;                        // W per slot of w: w_batch n / lanes
    uint32_t frame_mask, log_n, g;           // n / lanes - 1; g odd, below 2n (GALOIS only)
    uint32_t w_broadcast, accumulate;
};

__device__ __forceinline__ uint64_t mul_add_lanes(uint64_t w, uint64_t b, bool has_old, uint64_t old, const prime_consts& k, uint64_t q2) {
    return weighted_finish(ring_reduce(b, k.q, q2), true, w, has_old, old, k.q, q2, k.mu_hi, k.mu_lo);
}
__device__ __forceinline__ ulonglong2 mul_add_lanes(ulonglong2 w, ulonglong2 b, bool has_old, ulonglong2 old, const prime_consts& k, uint64_t q2) {
    return make_ulonglong2(mul_add_lanes(w.x, b.x, has_old, old.x, k, q2), mul_add_lanes(w.y, b.y, has_old, old.y, k, q2));
}

template <bool GALOIS, class W>
__global__ void ring_mul_add_kernel(const W* w, const W* b, W* c, const prime_consts* __restrict__ consts, mul_add_args ga) {
    constexpr int kLanes = sizeof(W) / 8;
    const ring_args& g = ga.in;
    const uint32_t slot = blockIdx.y;
    const prime_consts k = consts[g.first + slot];
    const uint64_t q2 = k.q << 1;
    const uint64_t off = (uint64_t)slot * g.per_prime;
    const W* wp = w + (uint64_t)slot * ga.w_prime;
    const bool has_old = ga.accumulate != 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.per_prime; i += (uint64_t)gridDim.x * blockDim.x) {
        bool swap = false;
        uint64_t bi = i;
        if constexpr (GALOIS) bi = galois_read_index<kLanes>(i, ga.frame_mask, ga.log_n, ga.g, swap);
        const W x = wp[ga.w_broadcast ? (i & ga.frame_mask) : i], y = b[off + bi];
        W old{};
        if (has_old) old = c[off + i];
        c[off + i] = mul_add_lanes(x, inner_gather(y, swap), has_old, old, k, q2);
    }
}

}  // namespace agx
