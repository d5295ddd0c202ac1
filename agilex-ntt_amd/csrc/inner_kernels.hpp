// inner_kernels.hpp -- the kernel of agx_ntt_inner_product / _inner_product_galois, and the Galois index text (galois_read_index, inner_gather) that every
// gathered streaming kernel reads through (ring_kernels.hpp, weighted_kernels.hpp).  Compiled in ntt_kernels.hip.  The accumulate-and-reduce step is
// csrc/inner_reduce.hpp, which tests/inner_selftest.cpp compiles too.
//
// A streaming kernel: no LDS, no barrier, no table; blockIdx.y is the slot of a prime in the call's list, grid-stride over the slot's batch x n words.  W is one
// word or a 16-byte pair (all three bases 16-byte aligned; n is even, so every stride below is a whole number of pairs).
#pragma once
#include "ntt_kernels.hpp"
#include "modarith.hpp"
#include "inner_reduce.hpp"

#include <type_traits>

namespace agx {

struct inner_args {
    uint64_t per_prime;                      // W per slot of a and c: batch n / lanes
    uint64_t a_term, c_out;                  // strides in W: A per_prime
    uint64_t b_prime, b_out, b_term;         // key strides in W: bhat_batch n / lanes, A b_prime, outputs b_out
    uint32_t frame_mask, broadcast;          // n / lanes - 1; 1: the key index is the position within the frame
    uint32_t terms, split, skip;             // slot y serves plan prime y (y < split) or y + skip: Q followed by special primes that lie apart
};

// the gathered instances' arguments: the un-gathered ones keep inner_args as it is
struct inner_galois_args {
    inner_args in;
    uint32_t log_n, g;                       // g odd, below 2n
};

__device__ __forceinline__ const inner_args& inner_part(const inner_args& g) { return g; }
__device__ __forceinline__ const inner_args& inner_part(const inner_galois_args& ga) { return ga.in; }

__device__ __forceinline__ void inner_lanes(acc128* s, uint64_t a, uint64_t b, uint64_t q, uint64_t q2) { acc_mul_add(s[0], reduce_4q(a, q, q2), reduce_4q(b, q, q2)); }
__device__ __forceinline__ void inner_lanes(acc128* s, ulonglong2 a, ulonglong2 b, uint64_t q, uint64_t q2) {
    acc_mul_add(s[0], reduce_4q(a.x, q, q2), reduce_4q(b.x, q, q2));
    acc_mul_add(s[1], reduce_4q(a.y, q, q2), reduce_4q(b.y, q, q2));
}
__device__ __forceinline__ void inner_store(uint64_t* p, const acc128* s, const prime_consts& k) { *p = acc_reduce(s[0], k.q, k.mu_hi, k.mu_lo); }
__device__ __forceinline__ void inner_store(ulonglong2* p, const acc128* s, const prime_consts& k) {
    *p = make_ulonglong2(acc_reduce(s[0], k.q, k.mu_hi, k.mu_lo), acc_reduce(s[1], k.q, k.mu_hi, k.mu_lo));
}

// A gathered kernel reads an operand through pi(i) = brev((g brev(i) + (g-1)/2) mod n), the permutation of automorphism_ntt_kernel.  An aligned block of 2^m
// output positions reads one aligned block of 2^m input positions, so a wave that produces 64 consecutive W reads one aligned 512-byte (pair form: 1 KiB)
// segment in permuted lane order.  In the pair form the output pair (2i, 2i+1) reads the input pair (2j, 2j+1) with the halves swapped iff the low bit of
// pi(2i) is set -- the argument written at automorphism_ntt_x2_kernel.
__device__ __forceinline__ uint64_t inner_gather(uint64_t v, bool) { return v; }
__device__ __forceinline__ ulonglong2 inner_gather(ulonglong2 v, bool swap) { return swap ? make_ulonglong2(v.y, v.x) : v; }
// the index text: work item i (in W of kLanes words, w its position within the frame) reads the W at the returned index, `swap`: with its halves exchanged
template <int kLanes>
__device__ __forceinline__ uint64_t galois_read_index(uint64_t i, uint32_t frame_mask, uint32_t log_n, uint32_t g, bool& swap) {
    const uint32_t mask = (1u << log_n) - 1u, shift = 32u - log_n, half = (g - 1u) >> 1;
    const uint32_t w = (uint32_t)i & frame_mask;      // the position within the frame, in W; its first word is w kLanes (even in pair form)
    const uint32_t j = __brev((g * (__brev(w * kLanes) >> shift) + half) & mask) >> shift;      // g < 2^16, brev < 2^15
    swap = kLanes == 2 && (j & 1u);
    return (i - w) + j / kLanes;
}

// c_o[i] = sum_t a_t[GALOIS ? pi(i) : i] o bhat_{t,o}[i] mod q on NTT-form frames; the key and c stay at natural positions.  Inputs in [0, 4q) are reduced
// first, the products are summed in 128 bits and reduced once (inner_reduce.hpp has the range argument).  terms and OUT are wave-uniform.  The terms go in
// groups of up to four: the loads of a group -- 4 words of a and 4 OUT of the key, per lane of W -- are all issued before the arithmetic on them, and the
// unrolled next group's loads do not depend on it; a group of sixteen would hold 48 W in registers.  pi is formed once per work item and serves every term,
// since the terms of a differ by a stride only.  A broadcast key (one frame per prime) is re-read by every frame: the repeats hit L2, nothing is kept across
// frames.  A twin that held the key words in registers across eight frames was built and measured (profiles/r10_keyswitch.md): 1 ... 3 % slower at n = 4096,
// 3 ... 8 % faster at n = 16384 with a spill in its two-output pair form; deleted.  The host sends g = 1 to the un-gathered instances.
template <bool GALOIS, int OUT, class W>
__global__ void inner_product_kernel(const W* __restrict__ a, const W* __restrict__ bhat, W* __restrict__ c, const prime_consts* __restrict__ consts,
                                     std::conditional_t<GALOIS, inner_galois_args, inner_args> ga) {
    constexpr int kLanes = sizeof(W) / 8, kGroup = 4;
    const inner_args& g = inner_part(ga);
    const uint32_t slot = blockIdx.y;
    const prime_consts k = consts[slot < g.split ? slot : slot + g.skip];
    const uint64_t q2 = k.q << 1;
    const W* ap = a + (uint64_t)slot * g.per_prime;
    const W* bp = bhat + (uint64_t)slot * g.b_prime;
    W* cp = c + (uint64_t)slot * g.per_prime;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.per_prime; i += (uint64_t)gridDim.x * blockDim.x) {
        bool swap = false;
        uint64_t ai = i;
        if constexpr (GALOIS) ai = galois_read_index<kLanes>(i, g.frame_mask, ga.log_n, ga.g, swap);
        const uint64_t bi = g.broadcast ? (i & g.frame_mask) : i;
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
        for (int o = 0; o < OUT; ++o) inner_store(cp + o * g.c_out + i, s[o], k);
    }
}

}  // namespace agx
