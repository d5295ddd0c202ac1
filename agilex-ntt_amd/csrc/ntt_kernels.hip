// ntt_kernels.hip -- gfx950 (CDNA4, wave64) kernels for the batched negacyclic NTT.
//
// The radix-2 / LDS-resident kernels: one workgroup per frame, one butterfly stage per barrier.
// They perform exactly the reference's operation sequence (src/kernel/ntt.cpp:147-180,
// 298-300, 331-369, 377-394), so they are bit-identical to it even on out-of-contract
// tables.  Any power-of-two n; the always-available fallback.  The register-blocked kernels
// (the throughput path) live in rb_frame.hpp / rb_kernels.hpp and the reg_*.hip registry groups.
//
// No MFMA: this is 64-bit integer modular arithmetic (v_mad_u64_u32 / v_mul_hi_u32), bounded
// by VALU integer multiply issue and HBM bandwidth.
#include "rb_registry.hpp"
#include "modarith.hpp"
#include "inner_reduce.hpp"
#include "moddown_arith.hpp"      // the two per-word steps of AGX_RESCALE_ROUND in moddown_coeff_round_kernel
#include "bfv_conv_arith.hpp"     // the per-word steps of agx_ntt_basis_extend_exact / _mont in basis_aux_coeff_kernel
#include "bfv_quotient_arith.hpp" // those of agx_ntt_basis_quotient in basis_quotient_kernel

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>

namespace agx {

extern __shared__ __attribute__((aligned(16))) unsigned char agx_dyn_lds[];

static constexpr int kMaxLdsLog = 14;  // radix-2 kernels: 16384 coefficients = 128 KiB of the CU's 160 KiB LDS; n = 32768 runs as two blocks + one global stage

// ---------------------------------------------------------------------------------------
// radix-2 forward, LDS resident.  Block = one sub-transform of 2^nb_log coefficients:
// sub-block `blk` of the 2^split_log contiguous blocks a frame falls into after the first
// split_log stages (done by fwd_global_stage).  split_log = 0 -> the whole frame.
// ---------------------------------------------------------------------------------------
__global__ void fwd_radix2_lds(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                               const prime_consts* __restrict__ consts, const twpair* __restrict__ tw,
                               uint32_t log_n, uint32_t nb_log, uint32_t split_log,
                               int64_t prime_stride, int64_t poly_stride) {
    uint64_t* x = reinterpret_cast<uint64_t*>(agx_dyn_lds);
    const uint32_t nb = 1u << nb_log;
    const uint32_t prime = blockIdx.y;
    const uint64_t poly = blockIdx.x >> split_log;
    const uint32_t blk = blockIdx.x & ((1u << split_log) - 1u);
    const uint64_t q = consts[prime].q, q2 = q << 1;
    const twpair* twp = tw + ((size_t)prime << log_n);
    const int64_t base = (int64_t)prime * prime_stride + (int64_t)poly * poly_stride + ((int64_t)blk << nb_log);

    for (uint32_t e = threadIdx.x; e < nb; e += blockDim.x) x[e] = in[base + e];

    uint32_t t_log = nb_log - 1;
    for (uint32_t m = 1u << split_log; m < (1u << log_n); m <<= 1, --t_log) {
        __syncthreads();
        const uint32_t t = 1u << t_log;
        const uint32_t m_local = m >> split_log;
        for (uint32_t bf = threadIdx.x; bf < (nb >> 1); bf += blockDim.x) {
            const uint32_t i = bf >> t_log, j = bf & (t - 1);
            const uint32_t pos = (i << (t_log + 1)) + j;
            const twpair w = twp[m + blk * m_local + i];   // ntt.cpp:298-300
            uint64_t a = x[pos], b = x[pos + t];
            ct_butterfly(a, b, w.x, w.y, q, q2);
            if (t == 1) {                                    // ntt.cpp:377-394
                a = reduce_4q(a, q, q2);
                b = reduce_4q(b, q, q2);
            }
            x[pos] = a;
            x[pos + t] = b;
        }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < nb; e += blockDim.x) out[base + e] = x[e];
}

// one forward stage straight through global memory (only for frames larger than the LDS slab).
// stage s (0 = first): m = 2^s groups, gap t = n / 2^(s+1).
__global__ void fwd_global_stage(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst,
                                 const prime_consts* __restrict__ consts, const twpair* __restrict__ tw,
                                 uint32_t log_n, uint32_t stage, uint64_t batch,
                                 int64_t prime_stride, int64_t poly_stride) {
    const uint32_t prime = blockIdx.y;
    const uint64_t q = consts[prime].q, q2 = q << 1;
    const twpair* twp = tw + ((size_t)prime << log_n);
    const uint32_t half_log = log_n - 1, t_log = log_n - 1 - stage, t = 1u << t_log, m = 1u << stage;
    const uint64_t total = batch << half_log;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t poly = g >> half_log;
        const uint32_t bf = (uint32_t)(g & ((1u << half_log) - 1u));
        const uint32_t i = bf >> t_log, j = bf & (t - 1);
        const int64_t pos = (int64_t)prime * prime_stride + (int64_t)poly * poly_stride + ((int64_t)i << (t_log + 1)) + j;
        const twpair w = twp[m + i];
        uint64_t a = src[pos], b = src[pos + t];
        ct_butterfly(a, b, w.x, w.y, q, q2);
        if (t == 1) { a = reduce_4q(a, q, q2); b = reduce_4q(b, q, q2); }
        dst[pos] = a;
        dst[pos + t] = b;
    }
}

// ---------------------------------------------------------------------------------------
// radix-2 inverse (Gentleman-Sande), LDS resident: stages t = 1 .. nb/2 of each 2^nb_log
// block; the remaining split_log stages (gaps >= nb) run in inv_global_stage.  The stage with
// m = 1 also multiplies by n^-1 and fully reduces.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void gs_last(uint64_t& a, uint64_t& b, const prime_consts& k, uint64_t q2) {
    const uint64_t s = a + b;            // < 4q: mul_shoup_lazy takes any 64-bit value
    const uint64_t d = a + q2 - b;
    a = csub(mul_shoup_lazy(s, k.n_inv, k.n_inv_p, k.q), k.q);
    b = csub(mul_shoup_lazy(d, k.w1n, k.w1n_p, k.q), k.q);
}

__global__ void inv_radix2_lds(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                               const prime_consts* __restrict__ consts, const twpair* __restrict__ itw,
                               uint32_t log_n, uint32_t nb_log, uint32_t split_log,
                               int64_t prime_stride, int64_t poly_stride) {
    uint64_t* x = reinterpret_cast<uint64_t*>(agx_dyn_lds);
    const uint32_t nb = 1u << nb_log;
    const uint32_t prime = blockIdx.y;
    const uint64_t poly = blockIdx.x >> split_log;
    const uint32_t blk = blockIdx.x & ((1u << split_log) - 1u);
    const prime_consts k = consts[prime];
    const uint64_t q = k.q, q2 = q << 1;
    const twpair* twp = itw + ((size_t)prime << log_n);
    const int64_t base = (int64_t)prime * prime_stride + (int64_t)poly * poly_stride + ((int64_t)blk << nb_log);

    for (uint32_t e = threadIdx.x; e < nb; e += blockDim.x) x[e] = csub(in[base + e], q2);  // [0,4q) -> [0,2q)

    uint32_t t_log = 0;
    for (uint32_t m = 1u << (log_n - 1); m >= (1u << split_log); m >>= 1, ++t_log) {
        __syncthreads();
        const uint32_t t = 1u << t_log;
        const uint32_t m_local = m >> split_log;
        for (uint32_t bf = threadIdx.x; bf < (nb >> 1); bf += blockDim.x) {
            const uint32_t i = bf >> t_log, j = bf & (t - 1);
            const uint32_t pos = (i << (t_log + 1)) + j;
            uint64_t a = x[pos], b = x[pos + t];
            if (m == 1) {
                gs_last(a, b, k, q2);
            } else {
                const twpair w = twp[m + blk * m_local + i];
                gs_butterfly(a, b, w.x, w.y, q, q2);
            }
            x[pos] = a;
            x[pos + t] = b;
        }
        if (m == 1) break;
    }
    __syncthreads();
    if (nb_log == 0) x[0] = csub(x[0], q);
    for (uint32_t e = threadIdx.x; e < nb; e += blockDim.x) out[base + e] = x[e];
}

__global__ void inv_global_stage(uint64_t* __restrict__ data, const prime_consts* __restrict__ consts,
                                 const twpair* __restrict__ itw, uint32_t log_n, uint32_t stage, uint64_t batch,
                                 int64_t prime_stride, int64_t poly_stride) {
    // `stage` counts like the forward pass: m = 2^stage groups, gap t = n / 2^(stage+1)
    const uint32_t prime = blockIdx.y;
    const prime_consts k = consts[prime];
    const uint64_t q = k.q, q2 = q << 1;
    const twpair* twp = itw + ((size_t)prime << log_n);
    const uint32_t half_log = log_n - 1, t_log = log_n - 1 - stage, t = 1u << t_log, m = 1u << stage;
    const uint64_t total = batch << half_log;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t poly = g >> half_log;
        const uint32_t bf = (uint32_t)(g & ((1u << half_log) - 1u));
        const uint32_t i = bf >> t_log, j = bf & (t - 1);
        const int64_t pos = (int64_t)prime * prime_stride + (int64_t)poly * poly_stride + ((int64_t)i << (t_log + 1)) + j;
        uint64_t a = data[pos], b = data[pos + t];
        if (m == 1) {
            gs_last(a, b, k, q2);
        } else {
            const twpair w = twp[m + i];
            gs_butterfly(a, b, w.x, w.y, q, q2);
        }
        data[pos] = a;
        data[pos + t] = b;
    }
}

// ---------------------------------------------------------------------------------------
// pointwise product and synthetic fill
// ---------------------------------------------------------------------------------------
__global__ void pointwise_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, uint64_t* __restrict__ c,
                                 const prime_consts* __restrict__ consts, uint64_t per_prime) {
    const uint32_t prime = blockIdx.y;
    const prime_consts k = consts[prime];
    const barrett128 bk{k.q, k.mu_hi, k.mu_lo};
    const uint64_t q2 = k.q << 1;
    const uint64_t off = (uint64_t)prime * per_prime;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_prime; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t u = reduce_4q(a[off + i], k.q, q2), v = reduce_4q(b[off + i], k.q, q2);
        c[off + i] = mul_mod_barrett(u, v, bk);
    }
}

// c <- c o bhat in place: element i of frame f of prime p meets bhat[p * bhat_prime_stride + f * bhat_poly_stride + i]
// (bhat_poly_stride = 0: every frame of a prime meets the same bhat frame); both may be lazy ([0,4q))
__global__ void pointwise_bhat_kernel(uint64_t* __restrict__ c, const uint64_t* __restrict__ bhat, const prime_consts* __restrict__ consts,
                                      uint32_t log_n, uint64_t per_prime, int64_t bhat_prime_stride, int64_t bhat_poly_stride) {
    const uint32_t prime = blockIdx.y;
    const prime_consts k = consts[prime];
    const barrett128 bk{k.q, k.mu_hi, k.mu_lo};
    const uint64_t q2 = k.q << 1;
    uint64_t* cp = c + (uint64_t)prime * per_prime;
    const uint64_t* bp = bhat + (int64_t)prime * bhat_prime_stride;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_prime; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t v = bp[(int64_t)(i >> log_n) * bhat_poly_stride + (int64_t)(i & ((1ull << log_n) - 1ull))];
        cp[i] = mul_mod_barrett(reduce_4q(cp[i], k.q, q2), reduce_4q(v, k.q, q2), bk);
    }
}

// agx_ntt_inner_product: c_o = sum_t a_t o bhat_{t,o} mod q on NTT-form frames.  A streaming kernel: no LDS, no barrier, no table; blockIdx.y is
// the slot of a prime in the call's list, grid-stride over the slot's batch x n words.  W is one word or a 16-byte pair (all three bases 16-byte
// aligned; n is even, so every stride below is a whole number of pairs).  Inputs in [0, 4q) are reduced first, the products are summed in 128
// bits and reduced once (inner_reduce.hpp has the range argument).  terms and OUT are wave-uniform.  The terms go in groups of up to four: the
// loads of a group -- 4 words of a and 4 OUT of the key, per lane of W -- are all issued before the arithmetic on them, and the unrolled next
// group's loads do not depend on it; a group of sixteen would hold 48 W in registers.  A broadcast key (one frame per prime) is re-read by every
// frame: the repeats hit L2, nothing is kept across frames.  A twin that held the key words in registers across eight frames was built and measured
// (profiles/r10_keyswitch.md): 1 ... 3 % slower at n = 4096, 3 ... 8 % faster at n = 16384 with a spill in its two-output pair form; deleted.
struct inner_args {
    uint64_t per_prime;                      // W per slot of a and c: batch n / lanes
    uint64_t a_term, c_out;                  // strides in W: A per_prime
    uint64_t b_prime, b_out, b_term;         // key strides in W: bhat_batch n / lanes, A b_prime, outputs b_out
    uint32_t frame_mask, broadcast;          // n / lanes - 1; 1: the key index is the position within the frame
    uint32_t terms, split, skip;             // slot y serves plan prime y (y < split) or y + skip: Q followed by special primes that lie apart
};

__device__ __forceinline__ void inner_lanes(acc128* s, uint64_t a, uint64_t b, uint64_t q, uint64_t q2) { acc_mul_add(s[0], reduce_4q(a, q, q2), reduce_4q(b, q, q2)); }
__device__ __forceinline__ void inner_lanes(acc128* s, ulonglong2 a, ulonglong2 b, uint64_t q, uint64_t q2) {
    acc_mul_add(s[0], reduce_4q(a.x, q, q2), reduce_4q(b.x, q, q2));
    acc_mul_add(s[1], reduce_4q(a.y, q, q2), reduce_4q(b.y, q, q2));
}
__device__ __forceinline__ void inner_store(uint64_t* p, const acc128* s, const prime_consts& k) { *p = acc_reduce(s[0], k.q, k.mu_hi, k.mu_lo); }
__device__ __forceinline__ void inner_store(ulonglong2* p, const acc128* s, const prime_consts& k) {
    *p = make_ulonglong2(acc_reduce(s[0], k.q, k.mu_hi, k.mu_lo), acc_reduce(s[1], k.q, k.mu_hi, k.mu_lo));
}

template <int OUT, class W>
__global__ void inner_product_kernel(const W* __restrict__ a, const W* __restrict__ bhat, W* __restrict__ c, const prime_consts* __restrict__ consts, inner_args g) {
    constexpr int kLanes = sizeof(W) / 8, kGroup = 4;
    const uint32_t slot = blockIdx.y;
    const prime_consts k = consts[slot < g.split ? slot : slot + g.skip];
    const uint64_t q2 = k.q << 1;
    const W* ap = a + (uint64_t)slot * g.per_prime;
    const W* bp = bhat + (uint64_t)slot * g.b_prime;
    W* cp = c + (uint64_t)slot * g.per_prime;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.per_prime; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t bi = g.broadcast ? (i & g.frame_mask) : i;
        acc128 s[OUT][kLanes];
        for (uint32_t t0 = 0; t0 < g.terms; t0 += kGroup) {
            W av[kGroup], bv[kGroup][OUT];
#pragma unroll
            for (int u = 0; u < kGroup; ++u)
                if (t0 + u < g.terms) {
                    av[u] = ap[(t0 + u) * g.a_term + i];
#pragma unroll
                    for (int o = 0; o < OUT; ++o) bv[u][o] = bp[(t0 + u) * g.b_term + o * g.b_out + bi];
                }
#pragma unroll
            for (int u = 0; u < kGroup; ++u)
                if (t0 + u < g.terms) {
#pragma unroll
                    for (int o = 0; o < OUT; ++o) inner_lanes(s[o], av[u], bv[u][o], k.q, q2);
                }
        }
#pragma unroll
        for (int o = 0; o < OUT; ++o) inner_store(cp + o * g.c_out + i, s[o], k);
    }
}

// agx_ntt_inner_product_galois: the same sum with a read through pi(i) = brev((g brev(i) + (g-1)/2) mod n), the permutation of
// automorphism_ntt_kernel below: c_o[i] = sum_t a_t[pi(i)] o bhat_{t,o}[i].  The key and c stay at natural positions.  The same grid-stride shape,
// groups of four terms and 128-bit sums as inner_product_kernel; pi is formed once per work item and serves every term, since the terms of a
// differ by a stride only.  An aligned block of 2^m output positions reads one aligned block of 2^m input positions, so a wave that produces 64
// consecutive W reads one aligned 512-byte (pair form: 1 KiB) segment of each term in permuted lane order.  In the pair form the output pair
// (2i, 2i+1) reads the input pair (2j, 2j+1) with the halves swapped iff the low bit of pi(2i) is set -- the argument written at
// automorphism_ntt_x2_kernel.  No LDS, no barrier, no table.  The host sends g = 1 to inner_product_kernel.
struct inner_galois_args {
    inner_args in;
    uint32_t log_n, g;                       // g odd, below 2n
};

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

template <int OUT, class W>
__global__ void inner_product_galois_kernel(const W* __restrict__ a, const W* __restrict__ bhat, W* __restrict__ c, const prime_consts* __restrict__ consts,
                                            inner_galois_args ga) {
    constexpr int kLanes = sizeof(W) / 8, kGroup = 4;
    const inner_args& g = ga.in;
    const uint32_t slot = blockIdx.y;
    const prime_consts k = consts[slot < g.split ? slot : slot + g.skip];
    const uint64_t q2 = k.q << 1;
    const W* ap = a + (uint64_t)slot * g.per_prime;
    const W* bp = bhat + (uint64_t)slot * g.b_prime;
    W* cp = c + (uint64_t)slot * g.per_prime;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.per_prime; i += (uint64_t)gridDim.x * blockDim.x) {
        bool swap;
        const uint64_t ai = galois_read_index<kLanes>(i, g.frame_mask, ga.log_n, ga.g, swap);
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

#include "ring_kernels.hpp"      // agx_ntt_add / _sub / _negate / _add_galois / _tensor: behind inner_gather and galois_read_index, which it reuses
#include "weighted_kernels.hpp"  // agx_ntt_keyswitch_accumulate_decomposed / agx_ntt_mul_add_galois: behind inner_args, inner_lanes and the ring arithmetic

namespace agx {

// agx_ntt_rescale, generic route, in the coefficient domain: out_i[k] <- (out_i[k] - u_i[k]) q_L^-1 mod q_i with u_i the lift of t[k] to q_i
// (rescale_lift).  out: dense [prime][batch][n] over the view's primes 0 .. P-2, values in [0,q_i) as the inverse leaves them; t: [batch][n]
// in [0,q_L), shared by the primes.
__global__ void rescale_coeff_kernel(uint64_t* __restrict__ out, const uint64_t* __restrict__ t, const prime_consts* __restrict__ consts,
                                     const rescale_consts* __restrict__ rcs, uint64_t per_prime, uint32_t round) {
    const uint32_t prime = blockIdx.y;
    const prime_consts k = consts[prime];
    const rescale_consts rc = rcs[prime];
    const barrett128 bk{k.q, k.mu_hi, k.mu_lo};
    const uint64_t h = round ? rc.h : 0, hq = round ? rc.h_mod_q : 0;
    uint64_t* op = out + (uint64_t)prime * per_prime;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_prime; i += (uint64_t)gridDim.x * blockDim.x)
        op[i] = rescale_finish<false>(op[i], rescale_lift(t[i], h, hq, rc.q_last, bk), rc.qlinv, rc.qlinv_p, k.q);
}

// ---------------------------------------------------------------------------------------
// agx_ntt_automorphism: a(X) -> a(X^g) mod (X^n + 1), g odd, dense [prime][batch][n], out of place
// ---------------------------------------------------------------------------------------
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

__device__ __forceinline__ uint64_t splitmix_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// element (prime, poly, i) = mix(mix(mix(seed ^ prime) + poly) + i) mod q : counter based, so the
// same coefficients come out whatever the sharding over devices
__global__ void fill_kernel(uint64_t* __restrict__ out, const prime_consts* __restrict__ consts,
                            uint32_t log_n, uint64_t batch, uint64_t first_poly, uint64_t seed) {
    const uint32_t prime = blockIdx.y;
    const uint64_t q = consts[prime].q;
    const uint64_t per_prime = batch << log_n;
    const uint64_t kp = splitmix_mix(seed ^ (uint64_t)prime);
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < per_prime; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t poly = first_poly + (g >> log_n), i = g & ((1ull << log_n) - 1ull);
        out[(uint64_t)prime * per_prime + g] = splitmix_mix(splitmix_mix(kp + poly) + i) % q;
    }
}

// ---------------------------------------------------------------------------------------
// host side: registry look-up and launches
// ---------------------------------------------------------------------------------------
namespace {

// every group of the registry, one per translation unit
template <class F>
void for_each_entry(F&& f) {
    const rb_span groups[] = {rb_entries_n4096(), rb_entries_s1024(), rb_entries_s2048(), rb_entries_s4096(), rb_entries_s8192(), rb_entries_s16384(), rb_entries_s32768(),
                              rb_entries_q32a(), rb_entries_q32b(), rb_entries_wp(), rb_entries_wp32(),
#ifdef AGX_DIAG
                              rb_entries_diag(),
#endif
    };
    for (const rb_span& g : groups)
        for (size_t i = 0; i < g.count; ++i) f(g.first[i]);
}

const rb_entry* rb_lookup(int id) {
    const rb_entry* hit = nullptr;
    for_each_entry([&](const rb_entry& e) { if (e.id == id && !hit) hit = &e; });
    return hit;
}

unsigned grid_1d(uint64_t work_items, unsigned threads) {
    uint64_t blocks = (work_items + threads - 1) / threads;
    if (blocks < 1) blocks = 1;
    if (blocks > 2048 * 8) blocks = 2048 * 8;  // grid-stride the rest
    return (unsigned)blocks;
}

template <typename F>
hipError_t set_lds_attr(F* fn, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

rb_selection regblock_select(uint32_t n, int config_id, int arith_level, int narrow_level) {
    rb_selection sel;
    int log_n = 0;
    while ((1u << log_n) < n) ++log_n;
    if (log_n < 1) return sel;
    // a 32-bit entry is legal when every modulus fits its tier and the tables honour the precon contract
    auto legal = [&](const rb_entry& c) { return c.arith <= arith_level && (c.narrow == 0 || (arith_level >= 1 && narrow_level >= (c.narrow == 2 ? 2 : 1))); };
    auto find = [&](int id) -> const rb_entry* {
        const rb_entry* c = rb_lookup(id);
        return c && c->log_n == log_n && legal(*c) ? c : nullptr;
    };
    if (config_id >= 0) {
        sel.main = find(config_id);
    } else {
        // tuned defaults, best first; the lazier arithmetic forms only when every modulus allows them
        static const int kDefaults[] = {260, 261, 262, 263, 264, 265, 266, 267, 230, 231, 232, 233, 234, 240, 241, 242, 243, 244,      // n = 2 ... 512, narrow moduli: wave-packed 32-bit kernels (tier 2, then tier 1)
                                        250, 251, 252, 253, 254, 255, 256, 257,                          // n = 2 ... 16: one lane per frame (fast, exact per size)
                                        200, 201, 202, 203, 204, 205, 206, 207, 208, 209, 210, 211, 212, 213, 214,      // n = 32 ... 512: wave-packed kernels (16q-lazy, fast, exact per size)
                                        130, 131, 132, 133, 134, 135, 136, 137, 138, 139, 140, 141,      // narrow moduli: 32-bit arithmetic (tier 2, then tier 1)
                                        93, 92, 91,                                                      // n = 4096: R = 3, 8 waves/SIMD (16q-lazy, fast, exact)
                                        150, 151, 152, 153, 154, 155, 156, 157, 158,                     // n = 1024 / 2048 / 8192: streamed single-frame kernels
                                        119, 117, 121, 120, 123, 122};                                  // n = 32768 / 16384
        for (int id : kDefaults)
            if ((sel.main = find(id))) break;
    }
    if (!sel.main || sel.main->fwd_companion <= 0) return sel;
    // tuned defaults among the forward companions: {companion, its twin for a narrower class of moduli}; the twin serves the plans whose moduli
    // allow it (same shape and table geometry; the companion's table is built by the entry that is chosen here)
    static const int kCompanionDefaults[][2] = {{159, 165}};      // n = 4096: moduli 2^60 - c, 0 < c < 2^28 (arithmetic level 3); which of id 165's two kernels
                                                                  // a launch gets (every c <= kQ60cSkipMaxC or not) is that entry's launch function's business
    int id = sel.main->fwd_companion;
    for (const auto& d : kCompanionDefaults)
        if (d[0] == id && find(d[1])) id = d[1];
    sel.forward_large = find(id);
    sel.min_frames = sel.main->fwd_companion_min_frames;
    return sel;
}

hipError_t kernels_init() {
    hipError_t e;
    const size_t big = (size_t)8 << kMaxLdsLog;
    if ((e = set_lds_attr(fwd_radix2_lds, big)) != hipSuccess) return e;
    if ((e = set_lds_attr(inv_radix2_lds, big)) != hipSuccess) return e;
    for_each_entry([&](const rb_entry& c) { if (e == hipSuccess) e = c.init(); });
    return e;
}

static unsigned radix2_threads(uint32_t nb) {
    uint32_t t = nb / 2;
    if (t < 64) t = 64;
    if (t > 1024) t = 1024;
    return t;
}

static uint32_t radix2_split(uint32_t log_n) { return log_n > (uint32_t)kMaxLdsLog ? log_n - kMaxLdsLog : 0; }      // stages run from global memory

int forward_radix2_launches(uint32_t log_n) { return (int)radix2_split(log_n) + 1; }
int inverse_radix2_launches(uint32_t log_n) { return (int)radix2_split(log_n) + 1; }

hipError_t launch_forward_radix2(const plan_view& pv, const uint64_t* in, uint64_t* out, const frame_layout& fl, hipStream_t s) {
    const uint32_t split = radix2_split(pv.log_n);
    const uint32_t nb_log = pv.log_n - split;
    const uint64_t* src = in;
    for (uint32_t st = 0; st < split; ++st) {
        dim3 grid(grid_1d(fl.batch << (pv.log_n - 1), 256), pv.num_primes);
        hipLaunchKernelGGL(fwd_global_stage, grid, dim3(256), 0, s, src, out, pv.consts, pv.tw, pv.log_n, st, fl.batch,
                           fl.prime_stride, fl.poly_stride);
        src = out;
    }
    dim3 grid((unsigned)(fl.batch << split), pv.num_primes);
    hipLaunchKernelGGL(fwd_radix2_lds, grid, dim3(radix2_threads(1u << nb_log)), (size_t)8 << nb_log, s, src, out, pv.consts,
                       pv.tw, pv.log_n, nb_log, split, fl.prime_stride, fl.poly_stride);
    return hipGetLastError();
}

hipError_t launch_inverse_radix2(const plan_view& pv, const uint64_t* in, uint64_t* out, const frame_layout& fl, hipStream_t s) {
    const uint32_t split = radix2_split(pv.log_n);
    const uint32_t nb_log = pv.log_n - split;
    dim3 grid((unsigned)(fl.batch << split), pv.num_primes);
    hipLaunchKernelGGL(inv_radix2_lds, grid, dim3(radix2_threads(1u << nb_log)), (size_t)8 << nb_log, s, in, out, pv.consts,
                       pv.itw, pv.log_n, nb_log, split, fl.prime_stride, fl.poly_stride);
    for (int st = (int)split - 1; st >= 0; --st) {
        dim3 g2(grid_1d(fl.batch << (pv.log_n - 1), 256), pv.num_primes);
        hipLaunchKernelGGL(inv_global_stage, g2, dim3(256), 0, s, out, pv.consts, pv.itw, pv.log_n, (uint32_t)st, fl.batch,
                           fl.prime_stride, fl.poly_stride);
    }
    return hipGetLastError();
}

hipError_t launch_pointwise_bhat(const plan_view& pv, uint64_t* c, const uint64_t* bhat, uint64_t batch, int64_t bhat_prime_stride,
                                 int64_t bhat_poly_stride, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    dim3 grid(grid_1d(per_prime, 256), pv.num_primes);
    hipLaunchKernelGGL(pointwise_bhat_kernel, grid, dim3(256), 0, s, c, bhat, pv.consts, pv.log_n, per_prime, bhat_prime_stride, bhat_poly_stride);
    return hipGetLastError();
}

hipError_t launch_pointwise(const plan_view& pv, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    dim3 grid(grid_1d(per_prime, 256), pv.num_primes);
    hipLaunchKernelGGL(pointwise_kernel, grid, dim3(256), 0, s, a, b, c, pv.consts, per_prime);
    return hipGetLastError();
}

// the 16-byte form serves when all three bases are 16-byte aligned
static bool inner_pairs(const uint64_t* a, const uint64_t* bhat, const uint64_t* c) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(bhat) | reinterpret_cast<uintptr_t>(c)) & 15u) == 0;
}

static inner_args inner_args_of(const plan_view& pv, const inner_primes& ip, uint64_t batch, uint64_t bhat_batch, uint32_t terms, uint32_t outputs, bool pairs) {
    const uint32_t shift = pairs ? 1 : 0;      // n >= 2 is even: a frame is a whole number of pairs
    inner_args g;
    g.per_prime = (batch << pv.log_n) >> shift;
    g.a_term = g.c_out = ip.count * g.per_prime;
    g.b_prime = (bhat_batch << pv.log_n) >> shift;
    g.b_out = ip.count * g.b_prime;
    g.b_term = outputs * g.b_out;
    g.frame_mask = (pv.n >> shift) - 1u;
    g.broadcast = bhat_batch == 1 && batch != 1 ? 1u : 0u;
    g.terms = terms, g.split = ip.split, g.skip = ip.skip;
    return g;
}

// the two kernel families of the inner products, by {outputs, word or pair}
struct inner_plain { template <int OUT, class W> static auto kernel() { return &inner_product_kernel<OUT, W>; } };
struct inner_galois { template <int OUT, class W> static auto kernel() { return &inner_product_galois_kernel<OUT, W>; } };

// one launch of a family's instance for {outputs 1 or 2} x {word or pair}; g: the family's argument block, per_prime its inner_args' work per slot
template <class Family, class Args>
static hipError_t launch_inner(const plan_view& pv, uint32_t slots, uint64_t per_prime, const uint64_t* a, const uint64_t* bhat, uint64_t* c, uint32_t outputs,
                               bool pairs, const Args& g, hipStream_t s) {
    const dim3 grid(grid_1d(per_prime, 256), slots);
    auto go = [&](auto kernel, auto* ap, auto* bp, auto* cp) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, ap, bp, cp, pv.consts, g); };
    if (pairs) {
        const ulonglong2 *a2 = reinterpret_cast<const ulonglong2*>(a), *b2 = reinterpret_cast<const ulonglong2*>(bhat);
        ulonglong2* c2 = reinterpret_cast<ulonglong2*>(c);
        if (outputs == 1) go(Family::template kernel<1, ulonglong2>(), a2, b2, c2);
        else go(Family::template kernel<2, ulonglong2>(), a2, b2, c2);
    } else {
        if (outputs == 1) go(Family::template kernel<1, uint64_t>(), a, bhat, c);
        else go(Family::template kernel<2, uint64_t>(), a, bhat, c);
    }
    return hipGetLastError();
}

hipError_t launch_inner_product_galois(const plan_view& pv, const inner_primes& ip, const uint64_t* a, const uint64_t* bhat, uint64_t* c, uint64_t batch,
                                       uint64_t bhat_batch, uint32_t terms, uint32_t outputs, uint32_t galois_elt, hipStream_t s) {
    if (galois_elt == 1) return launch_inner_product(pv, ip, a, bhat, c, batch, bhat_batch, terms, outputs, s);      // pi is the identity: the plain kernel
    const bool pairs = inner_pairs(a, bhat, c);
    const inner_galois_args g{inner_args_of(pv, ip, batch, bhat_batch, terms, outputs, pairs), pv.log_n, galois_elt};
    return launch_inner<inner_galois>(pv, ip.count, g.in.per_prime, a, bhat, c, outputs, pairs, g, s);
}

hipError_t launch_inner_product(const plan_view& pv, const inner_primes& ip, const uint64_t* a, const uint64_t* bhat, uint64_t* c, uint64_t batch,
                                uint64_t bhat_batch, uint32_t terms, uint32_t outputs, hipStream_t s) {
    const bool pairs = inner_pairs(a, bhat, c);
    const inner_args g = inner_args_of(pv, ip, batch, bhat_batch, terms, outputs, pairs);
    return launch_inner<inner_plain>(pv, ip.count, g.per_prime, a, bhat, c, outputs, pairs, g, s);
}

// The ring calls: one launch each over the plan primes [first, first + count), 256 threads, the 16-byte form when every base of the call allows it
template <class W, class Args>
static hipError_t launch_ring(void (*kernel)(const W*, const W*, W*, const prime_consts*, Args), const plan_view& pv, uint32_t count, uint64_t per_prime, const void* a,
                              const void* b, void* c, const Args& g, hipStream_t s) {
    hipLaunchKernelGGL(kernel, dim3(grid_1d(per_prime, 256), count), dim3(256), 0, s, static_cast<const W*>(a), static_cast<const W*>(b), static_cast<W*>(c), pv.consts, g);
    return hipGetLastError();
}

static hipError_t launch_ring_linear(const plan_view& pv, uint32_t first, uint32_t count, int op, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch, hipStream_t s) {
    const bool pairs = inner_pairs(a, b, c);      // a negation passes a for b
    const ring_args g{(batch << pv.log_n) >> (pairs ? 1 : 0), first};
    auto go = [&](auto kernel) { return launch_ring(kernel, pv, count, g.per_prime, a, b, c, g, s); };
    if (pairs) return op == RING_ADD ? go(&ring_linear_kernel<RING_ADD, ulonglong2>) : op == RING_SUB ? go(&ring_linear_kernel<RING_SUB, ulonglong2>) : go(&ring_linear_kernel<RING_NEG, ulonglong2>);
    return op == RING_ADD ? go(&ring_linear_kernel<RING_ADD, uint64_t>) : op == RING_SUB ? go(&ring_linear_kernel<RING_SUB, uint64_t>) : go(&ring_linear_kernel<RING_NEG, uint64_t>);
}

hipError_t launch_ring_add(const plan_view& pv, uint32_t first, uint32_t count, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch, hipStream_t s) {
    return launch_ring_linear(pv, first, count, RING_ADD, a, b, c, batch, s);
}
hipError_t launch_ring_sub(const plan_view& pv, uint32_t first, uint32_t count, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch, hipStream_t s) {
    return launch_ring_linear(pv, first, count, RING_SUB, a, b, c, batch, s);
}
hipError_t launch_ring_negate(const plan_view& pv, uint32_t first, uint32_t count, const uint64_t* a, uint64_t* c, uint64_t batch, hipStream_t s) {
    return launch_ring_linear(pv, first, count, RING_NEG, a, a, c, batch, s);
}

hipError_t launch_ring_add_galois(const plan_view& pv, uint32_t first, uint32_t count, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch,
                                  uint32_t galois_elt, hipStream_t s) {
    if (galois_elt == 1) return launch_ring_add(pv, first, count, a, b, c, batch, s);      // pi is the identity: the plain kernel
    const bool pairs = inner_pairs(a, b, c);
    const uint32_t shift = pairs ? 1 : 0;
    const ring_galois_args g{ring_args{(batch << pv.log_n) >> shift, first}, (pv.n >> shift) - 1u, pv.log_n, galois_elt};
    if (pairs) return launch_ring(&ring_add_galois_kernel<ulonglong2>, pv, count, g.in.per_prime, a, b, c, g, s);
    return launch_ring(&ring_add_galois_kernel<uint64_t>, pv, count, g.in.per_prime, a, b, c, g, s);
}

hipError_t launch_ring_tensor(const plan_view& pv, uint32_t first, uint32_t count, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch, hipStream_t s) {
    const bool pairs = inner_pairs(a, b, c);      // a component lies count batch n words behind the one before: an even number
    const uint64_t per_prime = (batch << pv.log_n) >> (pairs ? 1 : 0);
    const ring_tensor_args g{per_prime, count * per_prime, first};
    if (pairs) return launch_ring(&ring_tensor_kernel<ulonglong2>, pv, count, per_prime, a, b, c, g, s);
    return launch_ring(&ring_tensor_kernel<uint64_t>, pv, count, per_prime, a, b, c, g, s);
}

// The weighted, accumulating inner product of a key switch (two outputs, the key one frame per prime): one launch of inner_weighted_kernel; g = 1 takes
// its un-gathered instance.  The 16-byte form serves when ext, the key, acc and (where there is one) the weight are all 16-byte aligned.
hipError_t launch_inner_weighted(const plan_view& pv, const inner_primes& ip, const uint64_t* a, const uint64_t* bhat, const uint64_t* weight, uint64_t weight_batch,
                                 uint64_t* acc, uint64_t batch, uint32_t terms, uint32_t galois_elt, bool accumulate, hipStream_t s) {
    const uint64_t* wt = weight ? weight : a;      // no weight: never read; a valid base keeps the slot arithmetic defined
    const bool pairs = inner_pairs(a, bhat, acc) && inner_pairs(wt, wt, wt);
    const uint32_t shift = pairs ? 1 : 0;
    weighted_args g;
    g.in = inner_args_of(pv, ip, batch, 1, terms, 2, pairs);
    g.w_prime = weight ? (weight_batch << pv.log_n) >> shift : 0;
    g.log_n = pv.log_n, g.g = galois_elt;
    g.has_weight = weight ? 1u : 0u, g.w_broadcast = weight_batch == 1 ? 1u : 0u, g.accumulate = accumulate ? 1u : 0u;
    const dim3 grid(grid_1d(g.in.per_prime, 256), ip.count);
    auto go = [&](auto kernel, auto* ap, auto* bp, auto* wp, auto* cp) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, ap, bp, wp, cp, pv.consts, g); };
    if (pairs) {
        const ulonglong2 *a2 = reinterpret_cast<const ulonglong2*>(a), *b2 = reinterpret_cast<const ulonglong2*>(bhat), *w2 = reinterpret_cast<const ulonglong2*>(wt);
        ulonglong2* c2 = reinterpret_cast<ulonglong2*>(acc);
        if (galois_elt == 1) go(&inner_weighted_kernel<false, ulonglong2>, a2, b2, w2, c2);
        else go(&inner_weighted_kernel<true, ulonglong2>, a2, b2, w2, c2);
    } else {
        if (galois_elt == 1) go(&inner_weighted_kernel<false, uint64_t>, a, bhat, wt, acc);
        else go(&inner_weighted_kernel<true, uint64_t>, a, bhat, wt, acc);
    }
    return hipGetLastError();
}

hipError_t launch_ring_mul_add_galois(const plan_view& pv, uint32_t first, uint32_t count, const uint64_t* w, uint64_t w_batch, const uint64_t* b, uint64_t* c,
                                      uint64_t batch, uint32_t galois_elt, bool accumulate, hipStream_t s) {
    const bool pairs = inner_pairs(w, b, c);
    const uint32_t shift = pairs ? 1 : 0;
    const mul_add_args g{ring_args{(batch << pv.log_n) >> shift, first}, (w_batch << pv.log_n) >> shift, (pv.n >> shift) - 1u, pv.log_n, galois_elt,
                         w_batch == 1 ? 1u : 0u, accumulate ? 1u : 0u};
    if (pairs) return galois_elt == 1 ? launch_ring(&ring_mul_add_kernel<false, ulonglong2>, pv, count, g.in.per_prime, w, b, c, g, s)
                                      : launch_ring(&ring_mul_add_kernel<true, ulonglong2>, pv, count, g.in.per_prime, w, b, c, g, s);
    return galois_elt == 1 ? launch_ring(&ring_mul_add_kernel<false, uint64_t>, pv, count, g.in.per_prime, w, b, c, g, s)
                           : launch_ring(&ring_mul_add_kernel<true, uint64_t>, pv, count, g.in.per_prime, w, b, c, g, s);
}

hipError_t launch_rescale_coeff(const plan_view& pv, uint64_t* out, const uint64_t* t, uint64_t batch, bool round, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    dim3 grid(grid_1d(per_prime, 256), pv.num_primes);
    hipLaunchKernelGGL(rescale_coeff_kernel, grid, dim3(256), 0, s, out, t, pv.consts, pv.rescale, per_prime, round ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_automorphism_ntt(const plan_view& pv, const uint64_t* in, uint64_t* out, uint64_t batch, uint32_t g, hipStream_t s) {
    const uint64_t total = ((uint64_t)pv.num_primes * batch) << pv.log_n;
    if (((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0) {
        hipLaunchKernelGGL(automorphism_ntt_x2_kernel, dim3(grid_1d(total >> 1, 256)), dim3(256), 0, s, reinterpret_cast<const ulonglong2*>(in),
                           reinterpret_cast<ulonglong2*>(out), pv.log_n, total >> 1, g);
    } else {
        hipLaunchKernelGGL(automorphism_ntt_kernel, dim3(grid_1d(total, 256)), dim3(256), 0, s, in, out, pv.log_n, total, g);
    }
    return hipGetLastError();
}

hipError_t launch_automorphism_coeff(const plan_view& pv, const uint64_t* in, uint64_t* out, uint64_t batch, uint32_t g, hipStream_t s) {
    uint32_t h = g;      // g^-1 mod 2n: Newton's iteration doubles the correct low bits (3 -> 6 -> 12 -> 24)
    for (int it = 0; it < 3; ++it) h *= 2u - g * h;
    h &= (2u << pv.log_n) - 1u;
    const uint64_t per_prime = batch << pv.log_n;
    dim3 grid(grid_1d(per_prime, 256), pv.num_primes);
    hipLaunchKernelGGL(automorphism_coeff_gather_kernel, grid, dim3(256), 0, s, in, out, pv.consts, pv.log_n, per_prime, h);
    return hipGetLastError();
}

// the SMAX a kernel templated on its source capacity is instantiated with for S sources (at most AGX_BASIS_MAX_SRC = 16), as a compile-time constant
template <class F>
static void with_smax(uint32_t S, F&& f) {
    if (S <= 1) f(std::integral_constant<int, 1>{});
    else if (S <= 2) f(std::integral_constant<int, 2>{});
    else if (S <= 4) f(std::integral_constant<int, 4>{});
    else if (S <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

hipError_t launch_basis_coeff(const plan_view& pv, const basis_view& bv, const uint64_t* x, uint64_t* out, uint64_t batch, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    const dim3 grid(grid_1d(per_prime, 256));
    with_smax(bv.src_count, [&](auto smax) {
        hipLaunchKernelGGL(basis_coeff_kernel<decltype(smax)::value>, grid, dim3(256), 0, s, x, out, pv.consts + bv.src_first, pv.consts + bv.dst_first, bv.dinv,
                           bv.mat, bv.src_count, bv.dst_count, per_prime);
    });
    return hipGetLastError();
}

hipError_t launch_basis_aux_coeff(const plan_view& pv, const basis_view& bv, const aux_view& av, bool exact, const uint64_t* x, const uint64_t* xaux, uint64_t* out,
                                  uint64_t batch, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    const dim3 grid(grid_1d(per_prime, 256));
    const aux_set& c = exact ? av.exact : av.mont;
    with_smax(bv.src_count, [&](auto smax) {
        if (exact)
            hipLaunchKernelGGL((basis_aux_coeff_kernel<decltype(smax)::value, true>), grid, dim3(256), 0, s, x, xaux, out, pv.consts + bv.src_first,
                               pv.consts + bv.dst_first, c.dinv, c.mat, av.row, c.corr, av.m, c.k, c.kp, bv.src_count, bv.dst_count, per_prime);
        else
            hipLaunchKernelGGL((basis_aux_coeff_kernel<decltype(smax)::value, false>), grid, dim3(256), 0, s, x, xaux, out, pv.consts + bv.src_first,
                               pv.consts + bv.dst_first, c.dinv, c.mat, av.row, c.corr, av.m, c.k, c.kp, bv.src_count, bv.dst_count, per_prime);
    });
    return hipGetLastError();
}

hipError_t launch_basis_quotient(const plan_view& pv, const basis_view& bv, const aux_view& av, const ulonglong2* qmat, const uint64_t* y, uint64_t* out, uint64_t batch,
                                 hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    const dim3 grid(grid_1d(per_prime, 256));
    with_smax(bv.src_count, [&](auto smax) {
        hipLaunchKernelGGL(basis_quotient_kernel<decltype(smax)::value>, grid, dim3(256), 0, s, y, out, pv.consts + bv.src_first, pv.consts + bv.dst_first, qmat,
                           av.exact.mat, av.row, av.exact.corr, av.m, av.exact.k, av.exact.kp, bv.src_count, bv.dst_count, per_prime);
    });
    return hipGetLastError();
}

hipError_t launch_moddown_coeff(const plan_view& pv, const basis_view& bv, uint64_t* out, const uint64_t* y, uint64_t batch, bool round, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    const dim3 grid(grid_1d(per_prime, 256));
    with_smax(bv.src_count, [&](auto smax) {
        if (round)
            hipLaunchKernelGGL(moddown_coeff_round_kernel<decltype(smax)::value>, grid, dim3(256), 0, s, out, y, pv.consts + bv.dst_first, bv.down_mat, bv.dall,
                               bv.src_count, bv.dst_count, per_prime, bv.round_src, bv.round_dst);
        else
            hipLaunchKernelGGL(moddown_coeff_kernel<decltype(smax)::value>, grid, dim3(256), 0, s, out, y, pv.consts + bv.dst_first, bv.down_mat, bv.dall, bv.src_count,
                               bv.dst_count, per_prime);
    });
    return hipGetLastError();
}

hipError_t launch_fill(const plan_view& pv, uint64_t* out, uint64_t batch, uint64_t first_poly, uint64_t seed, hipStream_t s) {
    dim3 grid(grid_1d(batch << pv.log_n, 256), pv.num_primes);
    hipLaunchKernelGGL(fill_kernel, grid, dim3(256), 0, s, out, pv.consts, pv.log_n, batch, first_poly, seed);
    return hipGetLastError();
}

}  // namespace agx
