// ring_kernels.hpp -- the kernels of agx_ntt_add, _sub, _negate, _add_galois and _tensor: linear arithmetic and the tensor product on NTT-form frames.
// Compiled in ntt_kernels.hip.  The gathered add reads through galois_read_index and inner_gather (inner_kernels.hpp: the index text and the pair form's
// half swap of the gathered inner product).  The per-word arithmetic is csrc/ring_arith.hpp, which tests/ring_selftest.cpp compiles too.
//
// All of them have the streaming shape of inner_product_kernel: blockIdx.y is the slot of a prime in the call's range and its constants are
// consts[first + slot]; grid-stride over the slot's batch x n words; no LDS, no barrier, no table.  W is one word, or a 16-byte pair when ALL bases of
// the call are 16-byte aligned (n is even, so a slot is a whole number of pairs).  Inputs in [0, 4q), outputs in [0, q).
// Pointers the calls allow to coincide carry no __restrict__: c with a or b in the linear kernel (its gathered instance: c with a), a with b in the tensor
// kernel.  A work item reads its own words of the operands c may equal before it writes them, and no other work item reads or writes those words.
#pragma once
#include "inner_kernels.hpp"
#include "ring_arith.hpp"

#include <type_traits>

namespace agx {

struct ring_args {
    uint64_t per_prime;      // W per slot: batch n / lanes
    uint32_t first;          // slot y serves plan prime first + y
};

template <int OP>
__device__ __forceinline__ uint64_t ring_word(uint64_t a, uint64_t b, uint64_t q, uint64_t q2) {
    if constexpr (OP == RING_ADD) return ring_add(a, b, q, q2);
    else if constexpr (OP == RING_SUB) return ring_sub(a, b, q, q2);
    else return ring_neg(a, q, q2);
}
template <int OP>
__device__ __forceinline__ uint64_t ring_lanes(uint64_t a, uint64_t b, uint64_t q, uint64_t q2) { return ring_word<OP>(a, b, q, q2); }
template <int OP>
__device__ __forceinline__ ulonglong2 ring_lanes(ulonglong2 a, ulonglong2 b, uint64_t q, uint64_t q2) {
    return make_ulonglong2(ring_word<OP>(a.x, b.x, q, q2), ring_word<OP>(a.y, b.y, q, q2));
}

// the gathered instance's arguments: the un-gathered ones keep ring_args as it is
struct ring_galois_args {
    ring_args in;
    uint32_t frame_mask, log_n, g;      // n / lanes - 1; g odd, below 2n
};

__device__ __forceinline__ const ring_args& ring_part(const ring_args& g) { return g; }
__device__ __forceinline__ const ring_args& ring_part(const ring_galois_args& ga) { return ga.in; }

// c = a + b, a - b or -a: 24 bytes per word, 16 for the negation (which reads no b).  GALOIS (the add alone): c[i] = a[i] + b[pi_g(i)] within every frame, b
// read through galois_read_index, formed once per work item; in the pair form an output pair reads one input pair, its halves swapped or not (inner_gather).
// There c may be a and touches b nowhere.  The host sends g = 1 to the un-gathered instance.
template <int OP, bool GALOIS, class W>
__global__ void ring_linear_kernel(const W* a, const W* b, W* c, const prime_consts* __restrict__ consts, std::conditional_t<GALOIS, ring_galois_args, ring_args> ga) {
    static_assert(!GALOIS || OP == RING_ADD, "the add alone has a gathered instance");
    const ring_args& g = ring_part(ga);
    const uint32_t slot = blockIdx.y;
    const uint64_t q = consts[g.first + slot].q, q2 = q << 1;
    const uint64_t off = (uint64_t)slot * g.per_prime;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.per_prime; i += (uint64_t)gridDim.x * blockDim.x) {
        if constexpr (GALOIS) {
            bool swap;
            const uint64_t bi = galois_read_index<sizeof(W) / 8>(i, ga.frame_mask, ga.log_n, ga.g, swap);
            const W x = a[off + i], y = b[off + bi];
            c[off + i] = ring_lanes<OP>(x, inner_gather(y, swap), q, q2);
        } else {
            const W x = a[off + i];
            W y = x;
            if constexpr (OP != RING_NEG) y = b[off + i];
            c[off + i] = ring_lanes<OP>(x, y, q, q2);
        }
    }
}

// (c_0, c_1, c_2) = (a_0 o b_0, a_0 o b_1 + a_1 o b_0, a_1 o b_1): a, b [2][count][batch][n], c [3][count][batch][n].  The four loads of a work item are
// issued before any arithmetic on them, three stores per lane of W: 56 bytes per word.  Four products, the cross term summed in 128 bits and reduced once
// (ring_arith.hpp).  c touches neither operand, so it alone is __restrict__; a and b may be one buffer (squaring).
struct ring_tensor_args {
    uint64_t per_prime;      // W per slot
    uint64_t part;           // W between the components of an operand: count per_prime
    uint32_t first;
};

__device__ __forceinline__ void tensor_lanes(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1, const prime_consts& k, uint64_t& c0, uint64_t& c1, uint64_t& c2) {
    ring_tensor(a0, a1, b0, b1, k.q, k.mu_hi, k.mu_lo, c0, c1, c2);
}
__device__ __forceinline__ void tensor_lanes(ulonglong2 a0, ulonglong2 a1, ulonglong2 b0, ulonglong2 b1, const prime_consts& k, ulonglong2& c0, ulonglong2& c1, ulonglong2& c2) {
    uint64_t x[3], y[3];      // ulonglong2's members are unsigned long long
    ring_tensor(a0.x, a1.x, b0.x, b1.x, k.q, k.mu_hi, k.mu_lo, x[0], x[1], x[2]);
    ring_tensor(a0.y, a1.y, b0.y, b1.y, k.q, k.mu_hi, k.mu_lo, y[0], y[1], y[2]);
    c0 = make_ulonglong2(x[0], y[0]), c1 = make_ulonglong2(x[1], y[1]), c2 = make_ulonglong2(x[2], y[2]);
}

template <class W>
__global__ void ring_tensor_kernel(const W* a, const W* b, W* __restrict__ c, const prime_consts* __restrict__ consts, ring_tensor_args g) {
    const uint32_t slot = blockIdx.y;
    const prime_consts k = consts[g.first + slot];
    const uint64_t off = (uint64_t)slot * g.per_prime;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.per_prime; i += (uint64_t)gridDim.x * blockDim.x) {
        const W a0 = a[off + i], a1 = a[g.part + off + i], b0 = b[off + i], b1 = b[g.part + off + i];
        W c0, c1, c2;
        tensor_lanes(a0, a1, b0, b1, k, c0, c1, c2);
        c[off + i] = c0;
        c[g.part + off + i] = c1;
        c[2 * g.part + off + i] = c2;
    }
}

}  // namespace agx
