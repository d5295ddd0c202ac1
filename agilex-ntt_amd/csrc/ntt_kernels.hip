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
//
// The streaming kernels of the RNS calls (a grid-stride over one slot's batch x n words, no LDS, no barrier) are compiled here from headers of their own;
// this file holds their launchers with every other, and the registry look-up.
#include "rb_registry.hpp"
#include "modarith.hpp"
#include "inner_kernels.hpp"           // agx_ntt_inner_product / _inner_product_galois, and the Galois index text of every gathered kernel
#include "ring_kernels.hpp"            // agx_ntt_add / _sub / _negate / _add_galois / _tensor
#include "weighted_kernels.hpp"        // agx_ntt_keyswitch_accumulate_decomposed / agx_ntt_mul_add_galois
#include "automorphism_kernels.hpp"    // agx_ntt_automorphism
#include "basis_coeff_kernels.hpp"     // the coefficient-domain steps of agx_ntt_basis_extend / _extend_exact / _extend_mont / _quotient / _mod_down
#include "plain_kernels.hpp"           // agx_ntt_plain_scale_up / _lift / _scale_down
#include "sample_kernels.hpp"          // agx_ntt_sample_uniform / _ternary / _cbd
#include "ckks_kernels.hpp"            // agx_ntt_ckks_encode / _decode
#include "batch_kernels.hpp"           // agx_ntt_batch_encode / _decode

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>

namespace agx {

extern __shared__ __attribute__((aligned(16))) unsigned char agx_dyn_lds[];

static constexpr int kCkksLdsLog = 13;  // CKKS kernels: 8192 slots = two planes of 64 KiB; 16384 slots (n = 32768, full) exchange through global memory
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
    // the CKKS kernels' planes: 16 bytes per slot, up to kCkksLdsLog slots
    const size_t planes = (size_t)16 << kCkksLdsLog;
    if (e == hipSuccess) e = set_lds_attr(&ckks_encode_kernel<false>, planes);
    if (e == hipSuccess) e = set_lds_attr(&ckks_encode_kernel<true>, planes);      // the real components of 16384 slots
    if (e == hipSuccess) e = set_lds_attr(&ckks_decode_kernel<1, false>, planes);
    if (e == hipSuccess) e = set_lds_attr(&ckks_decode_kernel<2, false>, planes);
    if (e == hipSuccess) e = set_lds_attr(&ckks_decode_kernel<4, false>, planes);
    if (e == hipSuccess) e = set_lds_attr(&ckks_decode_kernel<8, false>, planes);
    if (e == hipSuccess) e = set_lds_attr(&ckks_decode_kernel<16, false>, planes);
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

// One launch of a streaming kernel: grid_1d(work_items, 256) blocks of 256 threads by `slots` rows (blockIdx.y: the slot of a prime; 1 for a kernel that does
// not read it), the kernel's own arguments behind
template <class... P, class... A>
static hipError_t launch_stream(void (*kernel)(P...), uint64_t work_items, uint32_t slots, hipStream_t s, const A&... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_1d(work_items, 256), slots), dim3(256), 0, s, args...);
    return hipGetLastError();
}

hipError_t launch_pointwise_bhat(const plan_view& pv, uint64_t* c, const uint64_t* bhat, uint64_t batch, int64_t bhat_prime_stride,
                                 int64_t bhat_poly_stride, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    return launch_stream(pointwise_bhat_kernel, per_prime, pv.num_primes, s, c, bhat, pv.consts, pv.log_n, per_prime, bhat_prime_stride, bhat_poly_stride);
}

hipError_t launch_pointwise(const plan_view& pv, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    return launch_stream(pointwise_kernel, per_prime, pv.num_primes, s, a, b, c, pv.consts, per_prime);
}

// The kernels templated on a word type W, on gathered or not and on a small number (outputs, an op): the 16-byte form serves when all three bases are 16-byte
// aligned
static bool inner_pairs(const uint64_t* a, const uint64_t* bhat, const uint64_t* c) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(bhat) | reinterpret_cast<uintptr_t>(c)) & 15u) == 0;
}
template <class W> static const W* words(const uint64_t* p) { return reinterpret_cast<const W*>(p); }
template <class W> static W* words(uint64_t* p) { return reinterpret_cast<W*>(p); }

// The instance a call gets, in with_smax's style: f(w, gathered, v) with w a value of the word type -- a 16-byte pair when `pairs`, else one word --,
// gathered a std::bool_constant and v, a std::integral_constant, the one of Vs that `value` is (a call without such a number: <0> and 0).  g = 1 takes the
// un-gathered instance: pi is the identity.  f launches and returns the status.
template <int... Vs, class F>
static hipError_t with_instance(bool pairs, uint32_t galois_elt, int value, F&& f) {
    hipError_t e = hipErrorInvalidValue;      // `value` is none of Vs: nothing is launched (the C boundary lets no such call through)
    auto pick = [&](auto w, auto gathered) { (void)((value == Vs && ((e = f(w, gathered, std::integral_constant<int, Vs>{})), true)) || ...); };
    auto word = [&](auto gathered) { if (pairs) pick(ulonglong2{}, gathered); else pick(uint64_t{}, gathered); };
    if (galois_elt == 1) word(std::false_type{});
    else word(std::true_type{});
    return e;
}

// the argument block of an instance: a gathered one takes the whole of ga, an un-gathered one its first member
template <bool GALOIS, class A>
static const auto& args_of(const A& ga) {
    if constexpr (GALOIS) return ga;
    else return ga.in;
}

// one launch of the shape (a, b, c, consts, args) over `slots` primes of per_prime W each
template <class W, class Args>
static hipError_t launch_abc(void (*kernel)(const W*, const W*, W*, const prime_consts*, Args), const plan_view& pv, uint32_t slots, uint64_t per_prime, const uint64_t* a,
                             const uint64_t* b, uint64_t* c, const Args& g, hipStream_t s) {
    return launch_stream(kernel, per_prime, slots, s, words<W>(a), words<W>(b), words<W>(c), pv.consts, g);
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

hipError_t launch_inner_product_galois(const plan_view& pv, const inner_primes& ip, const uint64_t* a, const uint64_t* bhat, uint64_t* c, uint64_t batch,
                                       uint64_t bhat_batch, uint32_t terms, uint32_t outputs, uint32_t galois_elt, hipStream_t s) {
    const bool pairs = inner_pairs(a, bhat, c);
    const inner_galois_args ga{inner_args_of(pv, ip, batch, bhat_batch, terms, outputs, pairs), pv.log_n, galois_elt};
    return with_instance<1, 2>(pairs, galois_elt, (int)outputs, [&](auto w, auto gathered, auto out) {
        return launch_abc(&inner_product_kernel<gathered, out, decltype(w)>, pv, ip.count, ga.in.per_prime, a, bhat, c, args_of<gathered>(ga), s);
    });
}

// The ring calls: one launch each over the plan primes [first, first + count), the 16-byte form when every base of the call allows it
hipError_t launch_ring_linear(const plan_view& pv, uint32_t first, uint32_t count, ring_op op, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch,
                              uint32_t galois_elt, hipStream_t s) {
    const bool pairs = inner_pairs(a, b, c);      // a negation passes a for b
    const uint32_t shift = pairs ? 1 : 0;
    const ring_galois_args ga{ring_args{(batch << pv.log_n) >> shift, first}, (pv.n >> shift) - 1u, pv.log_n, galois_elt};
    return with_instance<RING_ADD, RING_SUB, RING_NEG>(pairs, galois_elt, op, [&](auto w, auto gathered, auto opc) {
        if constexpr (gathered && opc != RING_ADD) return hipErrorInvalidValue;      // the add alone has a gathered instance
        else return launch_abc(&ring_linear_kernel<opc, gathered, decltype(w)>, pv, count, ga.in.per_prime, a, b, c, args_of<gathered>(ga), s);
    });
}

hipError_t launch_ring_tensor(const plan_view& pv, uint32_t first, uint32_t count, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch, hipStream_t s) {
    const bool pairs = inner_pairs(a, b, c);      // a component lies count batch n words behind the one before: an even number
    const uint64_t per_prime = (batch << pv.log_n) >> (pairs ? 1 : 0);
    const ring_tensor_args g{per_prime, count * per_prime, first};
    return with_instance<0>(pairs, 1, 0, [&](auto w, auto, auto) { return launch_abc(&ring_tensor_kernel<decltype(w)>, pv, count, per_prime, a, b, c, g, s); });
}

// The weighted, accumulating inner product of a key switch (two outputs, the key one frame per prime): one launch of inner_weighted_kernel.  The 16-byte
// form serves when ext, the key, acc and (where there is one) the weight are all 16-byte aligned.
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
    return with_instance<0>(pairs, galois_elt, 0, [&](auto w, auto gathered, auto) {
        using W = decltype(w);
        return launch_stream(&inner_weighted_kernel<gathered, W>, g.in.per_prime, ip.count, s, words<W>(a), words<W>(bhat), words<W>(wt), words<W>(acc), pv.consts, g);
    });
}

hipError_t launch_ring_mul_add_galois(const plan_view& pv, uint32_t first, uint32_t count, const uint64_t* w, uint64_t w_batch, const uint64_t* b, uint64_t* c,
                                      uint64_t batch, uint32_t galois_elt, bool accumulate, hipStream_t s) {
    const bool pairs = inner_pairs(w, b, c);
    const uint32_t shift = pairs ? 1 : 0;
    const mul_add_args g{ring_args{(batch << pv.log_n) >> shift, first}, (w_batch << pv.log_n) >> shift, (pv.n >> shift) - 1u, pv.log_n, galois_elt,
                         w_batch == 1 ? 1u : 0u, accumulate ? 1u : 0u};
    return with_instance<0>(pairs, galois_elt, 0, [&](auto wd, auto gathered, auto) {
        return launch_abc(&ring_mul_add_kernel<gathered, decltype(wd)>, pv, count, g.in.per_prime, w, b, c, g, s);
    });
}

hipError_t launch_rescale_coeff(const plan_view& pv, uint64_t* out, const uint64_t* t, uint64_t batch, bool round, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    return launch_stream(rescale_coeff_kernel, per_prime, pv.num_primes, s, out, t, pv.consts, pv.rescale, per_prime, round ? 1u : 0u);
}

hipError_t launch_automorphism_ntt(const plan_view& pv, const uint64_t* in, uint64_t* out, uint64_t batch, uint32_t g, hipStream_t s) {
    const uint64_t total = ((uint64_t)pv.num_primes * batch) << pv.log_n;
    if (inner_pairs(in, in, out)) return launch_stream(automorphism_ntt_x2_kernel, total >> 1, 1, s, words<ulonglong2>(in), words<ulonglong2>(out), pv.log_n, total >> 1, g);
    return launch_stream(automorphism_ntt_kernel, total, 1, s, in, out, pv.log_n, total, g);
}

hipError_t launch_automorphism_coeff(const plan_view& pv, const uint64_t* in, uint64_t* out, uint64_t batch, uint32_t g, hipStream_t s) {
    uint32_t h = g;      // g^-1 mod 2n: Newton's iteration doubles the correct low bits (3 -> 6 -> 12 -> 24)
    for (int it = 0; it < 3; ++it) h *= 2u - g * h;
    h &= (2u << pv.log_n) - 1u;
    const uint64_t per_prime = batch << pv.log_n;
    return launch_stream(automorphism_coeff_gather_kernel, per_prime, pv.num_primes, s, in, out, pv.consts, pv.log_n, per_prime, h);
}

// The coefficient-domain basis kernels: one thread per (frame, coefficient), no slots.
// the SMAX a kernel templated on its source capacity is instantiated with for S sources (at most AGX_BASIS_MAX_SRC = 16), as a compile-time constant
template <class F>
static hipError_t with_smax(uint32_t S, F&& f) {
    if (S <= 1) return f(std::integral_constant<int, 1>{});
    if (S <= 2) return f(std::integral_constant<int, 2>{});
    if (S <= 4) return f(std::integral_constant<int, 4>{});
    if (S <= 8) return f(std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, 16>{});
}

hipError_t launch_basis_coeff(const plan_view& pv, const basis_view& bv, const uint64_t* x, uint64_t* out, uint64_t batch, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    return with_smax(bv.src_count, [&](auto smax) {
        return launch_stream(&basis_coeff_kernel<smax>, per_prime, 1, s, x, out, pv.consts + bv.src_first, pv.consts + bv.dst_first, bv.dinv, bv.mat, bv.src_count,
                             bv.dst_count, per_prime);
    });
}

hipError_t launch_basis_aux_coeff(const plan_view& pv, const basis_view& bv, const aux_view& av, bool exact, const uint64_t* x, const uint64_t* xaux, uint64_t* out,
                                  uint64_t batch, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    const aux_set& c = exact ? av.exact : av.mont;
    return with_smax(bv.src_count, [&](auto smax) {
        return launch_stream(exact ? &basis_aux_coeff_kernel<smax, true> : &basis_aux_coeff_kernel<smax, false>, per_prime, 1, s, x, xaux, out, pv.consts + bv.src_first,
                             pv.consts + bv.dst_first, c.dinv, c.mat, av.row, c.corr, av.m, c.k, c.kp, bv.src_count, bv.dst_count, per_prime);
    });
}

hipError_t launch_basis_quotient(const plan_view& pv, const basis_view& bv, const aux_view& av, const ulonglong2* qmat, const uint64_t* y, uint64_t* out, uint64_t batch,
                                 hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    return with_smax(bv.src_count, [&](auto smax) {
        return launch_stream(&basis_quotient_kernel<smax>, per_prime, 1, s, y, out, pv.consts + bv.src_first, pv.consts + bv.dst_first, qmat, av.exact.mat, av.row,
                             av.exact.corr, av.m, av.exact.k, av.exact.kp, bv.src_count, bv.dst_count, per_prime);
    });
}

hipError_t launch_moddown_coeff(const plan_view& pv, const basis_view& bv, uint64_t* out, const uint64_t* y, uint64_t batch, bool round, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    return with_smax(bv.src_count, [&](auto smax) {
        if (round)
            return launch_stream(&moddown_coeff_round_kernel<smax>, per_prime, 1, s, out, y, pv.consts + bv.dst_first, bv.down_mat, bv.dall, bv.src_count, bv.dst_count,
                                 per_prime, bv.round_src, bv.round_dst);
        return launch_stream(&moddown_coeff_kernel<smax>, per_prime, 1, s, out, y, pv.consts + bv.dst_first, bv.down_mat, bv.dall, bv.src_count, bv.dst_count, per_prime);
    });
}

// The plaintext boundary: one thread per (frame, coefficient), no slots; the scale-down on its source capacity as the basis kernels above
hipError_t launch_plain_encode(const plan_view& pv, const plain_view& cv, bool lift, const uint64_t* m, uint64_t* out, uint64_t batch, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    return launch_stream(lift ? &plain_encode_kernel<true> : &plain_encode_kernel<false>, per_prime, 1, s, m, out, pv.consts + cv.q_first, lift ? cv.one : cv.up, cv.t, cv.h,
                         cv.one_p, cv.d, cv.dp, cv.q_count, per_prime);
}

hipError_t launch_plain_scale_down(const plan_view& pv, const plain_view& cv, const uint64_t* y, uint64_t* m, uint64_t batch, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    return with_smax(cv.q_count, [&](auto smax) {
        return launch_stream(&plain_scale_down_kernel<smax>, per_prime, 1, s, y, m, cv.row_t, cv.row_g, cv.t, cv.gamma, cv.g, cv.gp, cv.q_count, per_prime);
    });
}

hipError_t launch_plain_centred_reduce(const plan_view& pv, const plain_view& cv, const uint64_t* y, uint64_t* m, uint64_t f, uint64_t fp, uint64_t batch, hipStream_t s) {
    const uint64_t per_prime = batch << pv.log_n;
    return with_smax(cv.q_count, [&](auto smax) {
        return launch_stream(&plain_centred_reduce_kernel<smax>, per_prime, 1, s, y, m, cv.q, reinterpret_cast<const uint64_t*>(cv.tri), reinterpret_cast<const uint64_t*>(cv.radix_t),
                             cv.t, cv.d, f, fp, cv.q_count, per_prime);
    });
}

// Batching: one thread per word, or per pair of words where the contiguous side admits 16-byte accesses; no slots.  kBatchScatter names the side that ships:
// false, the gathered READ (out[w] = in[tab[w]]).  Building with -DAGX_BATCH_SCATTER (the Makefile's EXTRA) gives the other side, contiguous loads and scattered
// writes through the inverse table, for an A/B library: profiles/r21_batching.md has both beside a copy.
#ifdef AGX_BATCH_SCATTER
static constexpr bool kBatchScatter = true;
#else
static constexpr bool kBatchScatter = false;
#endif

hipError_t launch_batch_permute(uint32_t log_n, const batch_view& bv, bool encode, const uint64_t* in, uint64_t* out, uint64_t batch, hipStream_t s) {
    const uint64_t words = batch << log_n;
    // gathered: the table of the OUTPUT's order (encode writes words: word -> slot); scattered: the table of the INPUT's order (encode reads slots: slot -> word)
    const uint32_t* tab = encode != kBatchScatter ? bv.word_to_slot : bv.slot_to_word;
    const void* contiguous = kBatchScatter ? static_cast<const void*>(in) : static_cast<const void*>(out);
    if ((reinterpret_cast<uintptr_t>(contiguous) & 15u) == 0)
        return launch_stream(encode ? &batch_permute_kernel<true, true, kBatchScatter> : &batch_permute_kernel<false, true, kBatchScatter>, words >> 1, 1, s, in, out, tab, bv.t,
                             bv.one_p, log_n, words >> 1);
    return launch_stream(encode ? &batch_permute_kernel<true, false, kBatchScatter> : &batch_permute_kernel<false, false, kBatchScatter>, words, 1, s, in, out, tab, bv.t, bv.one_p,
                         log_n, words);
}

// The CKKS boundary: one workgroup per frame, s / 4 threads within [64, 1024]; the planes in LDS up to 2^kCkksLdsLog slots, beyond (n = 32768 with full
// slots) the GLOBAL instances with 1024 threads
static ckks_args ckks_args_of(uint32_t log_n, const ckks_view& cv, uint32_t log_s, uint32_t count, uint64_t batch) {
    return ckks_args{cv.tw, cv.q, reinterpret_cast<const uint64_t*>(cv.tri), reinterpret_cast<const uint64_t*>(cv.pow2), log_n, log_s, count, batch << log_n};
}

static unsigned ckks_threads(uint32_t log_s) {
    const uint32_t t = (1u << log_s) >> 2;
    return t < 64 ? 64 : t > 1024 ? 1024 : t;
}

hipError_t launch_ckks_encode(uint32_t log_n, const ckks_view& cv, const double* z, uint32_t log_s, double scale, uint64_t* out, uint64_t batch, uint32_t count, hipStream_t s) {
    const ckks_args a = ckks_args_of(log_n, cv, log_s, count, batch);
    const bool global = log_s > (uint32_t)kCkksLdsLog;
    const double inv_s = 1.0 / (double)(1u << log_s);
    hipLaunchKernelGGL(global ? &ckks_encode_kernel<true> : &ckks_encode_kernel<false>, dim3((unsigned)batch), dim3(ckks_threads(log_s)), (size_t)(global ? 8 : 16) << log_s, s,
                       reinterpret_cast<const double2*>(z), out, a, scale, inv_s);
    return hipGetLastError();
}

hipError_t launch_ckks_decode(uint32_t log_n, const ckks_view& cv, const uint64_t* x, uint32_t count, double scale, double* z, uint32_t log_s, uint64_t batch, hipStream_t s) {
    const ckks_args a = ckks_args_of(log_n, cv, log_s, count, batch);
    const bool global = log_s > (uint32_t)kCkksLdsLog;
    const double inv_delta = 1.0 / scale;
    return with_smax(count, [&](auto smax) {
        constexpr int S = decltype(smax)::value;
        auto kernel = global ? &ckks_decode_kernel<S, true> : &ckks_decode_kernel<S, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(ckks_threads(log_s)), global ? 0 : (size_t)16 << log_s, s, x, reinterpret_cast<double2*>(z), a, inv_delta);
        return hipGetLastError();
    });
}

// The samplers: one thread per cell of eight coefficients (a whole frame for n = 2 and 4); uniform over `count` slots, the small kinds walk their primes
hipError_t launch_sample(const plan_view& pv, sample_kind kind, const uint32_t key[8], uint64_t nonce, uint32_t eta, uint64_t* out, uint64_t batch, uint64_t frame_first,
                         uint32_t first, uint32_t count, hipStream_t s) {
    sample_key k;
    for (int i = 0; i < 8; ++i) k.w[i] = key[i];
    const uint64_t cells = batch << (pv.log_n > 3 ? pv.log_n - 3 : 0);
    const sample_shape g{pv.log_n, (uint32_t)frame_first, (uint32_t)nonce, (uint32_t)(nonce >> 32), cells, batch << pv.log_n};
    const bool pairs = inner_pairs(out, out, out);
    if (kind == SAMPLE_UNIFORM) return launch_stream(pairs ? &sample_uniform_kernel<true> : &sample_uniform_kernel<false>, cells, count, s, out, pv.consts, k, g, first);
    auto small = [&](auto cbd) {
        return launch_stream(pairs ? &sample_small_kernel<cbd, true> : &sample_small_kernel<cbd, false>, cells, 1, s, out, pv.consts + first, k, g, sample_eta_mask(eta), count);
    };
    return kind == SAMPLE_CBD ? small(std::true_type{}) : small(std::false_type{});
}

hipError_t launch_fill(const plan_view& pv, uint64_t* out, uint64_t batch, uint64_t first_poly, uint64_t seed, hipStream_t s) {
    return launch_stream(fill_kernel, batch << pv.log_n, pv.num_primes, s, out, pv.consts, pv.log_n, batch, first_poly, seed);
}

}  // namespace agx
