// sample_kernels.hpp -- the kernels of agx_ntt_sample_uniform (sample_uniform_kernel) and of agx_ntt_sample_ternary / _cbd (sample_small_kernel).  Compiled in
// ntt_kernels.hip.  The shape of plain_kernels.hpp: a grid-stride over the batch x cells of one slab, no table, no LDS, no barrier -- but one thread per CELL
// (eight consecutive coefficients of a frame, the candidates of one ChaCha20 block; the whole frame for n = 2 and 4), so a lane's words are 64 contiguous
// bytes, stored 16 bytes at a time where the base allows it.  The key arrives in the kernel arguments: state words 0 .. 11, w14 and w15 are wave-uniform
// (scalar registers), the sixteen working words and the eight results live in vector registers.  sample_arith.hpp has the definition and the steps.
#pragma once
#include "ntt_kernels.hpp"
#include "sample_arith.hpp"

namespace agx {

// what every sampling launch knows of its place: log2 n, the cells of a slab (batch x max(1, n / 8)) and its words (batch x n)
struct sample_shape {
    uint32_t log_n, frame_first;      // frame f of the launch is frame frame_first + f of the draw (below 2^32: checked at the C boundary)
    uint32_t nonce_lo, nonce_hi;
    uint64_t cells, per_prime;
};

// the W = min(8, n) words of a cell to p: 16-byte stores when PAIRS (the base is 16-byte aligned; W, frames and slabs are even numbers of words)
template <bool PAIRS>
__device__ __forceinline__ void sample_store(uint64_t* __restrict__ p, const uint64_t v[8], uint32_t W) {
    if constexpr (PAIRS) {
        ulonglong2* p2 = reinterpret_cast<ulonglong2*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if ((uint32_t)(2 * i) < W) p2[i] = make_ulonglong2(v[2 * i], v[2 * i + 1]);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if ((uint32_t)i < W) p[i] = v[i];
    }
}

// agx_ntt_sample_uniform: out dense [slots][batch][n], slab blockIdx.y under plan prime prime_first + blockIdx.y (consts: the WHOLE plan's), fully reduced.  A
// thread walks the blocks of its cell until its W words are accepted: one block where q fills its bit length, two or more where it does not.
template <bool PAIRS>
__global__ void sample_uniform_kernel(uint64_t* __restrict__ out, const prime_consts* __restrict__ consts, sample_key key, sample_shape g, uint32_t prime_first) {
    const uint32_t prime = prime_first + blockIdx.y;
    const uint64_t q = consts[prime].q, mask = sample_mask(q);
    const uint32_t log_c = g.log_n > 3 ? g.log_n - 3 : 0, W = g.log_n >= 3 ? 8u : 1u << g.log_n;
    uint64_t* base = out + (uint64_t)blockIdx.y * g.per_prime;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < g.cells; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t f = (uint32_t)(e >> log_c), c = (uint32_t)e & ((1u << log_c) - 1u);
        const uint32_t w12 = sample_w12(prime, c, 0), w13 = g.frame_first + f;
        uint64_t v[8];
        sample_uniform_cell([&](uint32_t k, uint32_t o[16]) { sample_block(key, w12 | k, w13, g.nonce_lo, g.nonce_hi, o); }, q, mask, W, v);
        sample_store<PAIRS>(base + ((uint64_t)f << g.log_n) + 8u * c, v, W);
    }
}

// agx_ntt_sample_ternary (CBD = false) and agx_ntt_sample_cbd: out dense [L][batch][n], slab i under plan prime prime_first + i (consts points at it), fully
// reduced.  A thread computes ONE block and the eight small values of its cell once and walks the L primes, as plain_encode_kernel does.
template <bool CBD, bool PAIRS>
__global__ void sample_small_kernel(uint64_t* __restrict__ out, const prime_consts* __restrict__ consts, sample_key key, sample_shape g, uint32_t eta_mask, uint32_t L) {
    const uint32_t log_c = g.log_n > 3 ? g.log_n - 3 : 0, W = g.log_n >= 3 ? 8u : 1u << g.log_n;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < g.cells; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t f = (uint32_t)(e >> log_c), c = (uint32_t)e & ((1u << log_c) - 1u);
        uint32_t o[16];
        sample_block(key, sample_w12(kSampleSmallTag, c, CBD ? kSampleCbdK : kSampleTernaryK), g.frame_first + f, g.nonce_lo, g.nonce_hi, o);
        int32_t s[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = CBD ? sample_cbd(sample_candidate(o, i), eta_mask) : sample_ternary(sample_candidate(o, i));
        uint64_t* p = out + ((uint64_t)f << g.log_n) + 8u * c;
        for (uint32_t i = 0; i < L; ++i, p += g.per_prime) {
            const uint64_t q = consts[i].q;
            uint64_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = sample_residue(s[j], q);
            sample_store<PAIRS>(p, v, W);
        }
    }
}

}  // namespace agx
