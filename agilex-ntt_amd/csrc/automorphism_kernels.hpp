// automorphism_kernels.hpp -- the kernels of agx_ntt_automorphism: a(X) -> a(X^g) mod (X^n + 1), g odd, dense [prime][batch][n], out of place.  Compiled in
// ntt_kernels.hip.  Streaming kernels: grid-stride, no LDS, no barrier, no table.
#pragma once
#include "ntt_kernels.hpp"
#include "modarith.hpp"

namespace agx {

// NTT form (bit-reversed order): out[p] = in[pi(p)], pi(p) = brev((g brev(p) + (g-1)/2) mod n), words moved unchanged (no modulus).
// The high bits of k only move the high bits of g k + c, so an aligned block of 2^m output positions reads one aligned block of 2^m
// input positions: a wave that writes consecutive words reads one contiguous segment in permuted lane order.  No LDS, no barrier.
// One thread per word over all primes * batch * n words, 64-bit offsets.
__global__ void automorphism_ntt_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint32_t log_n, uint64_t total,
                                        uint32_t g) {
    const uint32_t mask = (1u << log_n) - 1u, shift = 32u - log_n, c = (g - 1u) >> 1;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t p = (uint32_t)i & mask;
        const uint32_t k = (g * (__brev(p) >> shift) + c) & mask;      // g < 2^16, brev(p) < 2^15
        out[i] = in[(i - p) + (__brev(k) >> shift)];
    }
}

// The same with 16-byte accesses (both bases 16-byte aligned): the output pair (2i, 2i+1) reads the input pair (2j, 2j+1) -- the odd
// member's k is the even member's plus n/2, which after the odd factor g still flips the top bit only -- swapped iff that top bit,
// the low bit of pi(2i), is set.  One thread per pair.
__global__ void automorphism_ntt_x2_kernel(const ulonglong2* __restrict__ in, ulonglong2* __restrict__ out, uint32_t log_n, uint64_t pairs,
                                           uint32_t g) {
    const uint32_t mask = (1u << log_n) - 1u, shift = 32u - log_n, c = (g - 1u) >> 1;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t p = ((uint32_t)i << 1) & mask;
        const uint32_t j = __brev((g * (__brev(p) >> shift) + c) & mask) >> shift;
        const ulonglong2 v = in[(i - (p >> 1)) + (j >> 1)];
        out[i] = (j & 1u) ? make_ulonglong2(v.y, v.x) : v;
    }
}

// Coefficient form (natural order): out[i] = +-in[j mod n], j = h i mod 2n with h = g^-1 mod 2n, minus iff j >= n; inputs in [0,4q),
// outputs fully reduced (so -0 = 0)
__device__ __forceinline__ uint64_t automorphism_coeff_word(uint64_t v, bool negate, uint64_t q, uint64_t q2) {
    v = reduce_4q(v, q, q2);
    return negate ? (v ? q - v : 0) : v;
}

// Gathered straight from global memory, one thread per output word: a frame comes from HBM once and the stride-h repeats hit L2.  Staging
// the frame in LDS (coalesced load, barrier, permuted LDS read) was measured at n = 64 ... 16384 and is nowhere faster: 0.4 ... 8 % slower at
// n = 512 ... 4096, 9 % at n = 64, 32 ... 38 % at n = 16384, where one 128 KiB workgroup per CU cannot overlap its loads with its stores
// (profiles/r07_automorphism.md)
__global__ void automorphism_coeff_gather_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, const prime_consts* __restrict__ consts,
                                                 uint32_t log_n, uint64_t per_prime, uint32_t h) {
    const uint32_t prime = blockIdx.y;
    const uint64_t q = consts[prime].q, q2 = q << 1;
    const uint64_t off = (uint64_t)prime * per_prime;
    const uint32_t mask = (1u << log_n) - 1u, mask2 = (2u << log_n) - 1u;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < per_prime; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = (uint32_t)e & mask, j = (h * i) & mask2;
        out[off + e] = automorphism_coeff_word(in[off + (e - i) + (j & mask)], j > mask, q, q2);
    }
}

}  // namespace agx
