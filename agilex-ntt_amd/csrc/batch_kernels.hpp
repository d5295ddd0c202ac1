// batch_kernels.hpp -- the permutation kernel of agx_ntt_batch_encode and agx_ntt_batch_decode.  Compiled in ntt_kernels.hip.  The shape of the other
// streaming kernels: grid-stride over the batch x n words, dense layouts, no LDS, no barrier.  batch_arith.hpp has the per-word steps.
#pragma once
#include "ntt_kernels.hpp"
#include "batch_arith.hpp"

namespace agx {

// A permutation within every frame, tab a permutation of [0, n) (n entries of 32 bits, read coalesced: a lane reads the entries of its own contiguous words);
// REDUCE: the word is reduced modulo t on its way (encode: d_z holds any 64-bit words), else it is moved as it is (decode: the forward wrote it below t).
//   SCATTER = false   out[frame][w] = in[frame][tab[w]]: the READ is the gathered side, the stores are contiguous
//   SCATTER = true    out[frame][tab[w]] = in[frame][w]: the loads are contiguous, the WRITE is the scattered side (with the inverse table the same permutation)
// With PAIRS a lane takes two neighbouring words of the contiguous side in one 16-byte access, for a 16-byte aligned base on that side (n is even, so every
// frame then starts aligned); the other side's 8-byte accesses land wherever the table says, always inside the lane's own frame (batch_source).
// `items`: batch n words, or half as many pairs.  8 bytes read, 8 written and 4 of the table (from cache after the first frame) per word.  out touches in
// nowhere.  Which side ships is launch_batch_permute's (ntt_kernels.hip), by the measurement of profiles/r21_batching.md.
template <bool REDUCE, bool PAIRS, bool SCATTER>
__global__ void batch_permute_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, const uint32_t* __restrict__ tab, uint64_t t, uint64_t one_p,
                                     uint32_t log_n, uint64_t items) {
    const uint32_t mask = (1u << log_n) - 1;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (uint64_t)gridDim.x * blockDim.x) {
        if (PAIRS) {
            const uint64_t e = i << 1;
            const uint2 k = reinterpret_cast<const uint2*>(tab)[(uint32_t)(e & mask) >> 1];
            uint64_t a, b;
            if (SCATTER) {
                const ulonglong2 v = reinterpret_cast<const ulonglong2*>(in)[i];
                a = v.x, b = v.y;
            } else {
                a = in[batch_source(e, log_n, k.x)], b = in[batch_source(e, log_n, k.y)];
            }
            if (REDUCE) a = batch_reduce(a, one_p, t), b = batch_reduce(b, one_p, t);
            if (SCATTER) out[batch_source(e, log_n, k.x)] = a, out[batch_source(e, log_n, k.y)] = b;
            else reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(a, b);
        } else {
            const uint64_t other = batch_source(i, log_n, tab[(uint32_t)(i & mask)]);
            const uint64_t a = in[SCATTER ? i : other];
            out[SCATTER ? other : i] = REDUCE ? batch_reduce(a, one_p, t) : a;
        }
    }
}

}  // namespace agx
