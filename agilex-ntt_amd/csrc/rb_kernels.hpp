// rb_kernels.hpp -- the register-blocked kernels (forward, inverse, fused product; one workgroup per frame or a resident grid for the
// inverse of the large sizes) over rb2_frame (rb_frame.hpp), their launch glue and the registry-entry constructors.  Included by the
// reg_*.hip translation units, each of which instantiates one group of registry entries under its own namespace AGX_TU.
#pragma once
#include "rb_frame.hpp"
#include "host_math.hpp"
#include "moddown_arith.hpp"      // the two per-word steps of AGX_RESCALE_ROUND in moddown_round_rb2

// mulhat_rb2 of a shape tuned for 8 waves/SIMD (n = 4096: 64 VGPRs) is compiled for 6 (80 VGPRs): with bhat's 16 words per thread
// requested ahead of the last forward pass it needs 69-80 registers, 64 cost 12-92 bytes of scratch per lane, and 512-thread
// workgroups occupy a SIMD two waves at a time anyway (7 = 6).  Measured equal to the 8-wave late-request form with a bhat frame
// per frame and +1.5 % with a shared one (profiles/r05_mulntt.md).
#ifndef AGX_MULHAT_MAXW
#define AGX_MULHAT_MAXW 6
#endif
namespace agx {
namespace AGX_TU {

// the frame type of a kernel's packed ARITH parameter: bit 0 = fast (1) / exact (0) arithmetic, the option bits (rb_frame.hpp) above it
template <int L, int R, int ARITH>
using frame_of = rb2_frame<L, R, (ARITH & 1) == 1, (ARITH >> 1)>;

#define AGX_RB2_PROLOGUE                                                                          \
    using F = frame_of<L, R, ARITH>;                                                              \
    constexpr int C = F::C, T = F::T;                                                             \
    static_assert(T >= 64, "one frame must span whole waves");                                    \
    F f;                                                                                          \
    f.tid = threadIdx.x & (T - 1);                                                                \
    const uint32_t slot = threadIdx.x / T;                                                        \
    uint64_t fx = (uint64_t)blockIdx.x * PPB + slot;                                              \
    const bool live = fx < frames_x;                                                              \
    if (!live) fx = frames_x - 1;                         /* keep every thread on the barriers */ \
    const uint32_t prime = blockIdx.y;                                                            \
    f.init_consts(consts[prime].q, consts[prime].est);                                            \
    f.slab = reinterpret_cast<uint64_t*>(agx_dyn_lds) + (size_t)slot * F::slab_elems;             \
    const int64_t base = (int64_t)prime * prime_stride + (int64_t)fx * poly_stride

template <int L, int R, int PPB, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)) * PPB, MINW)
fwd_rb2(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
        const prime_consts* __restrict__ consts, const twpair* __restrict__ tw_rb,
        uint32_t pairs_per_prime, uint64_t frames_x,
        int64_t prime_stride, int64_t poly_stride, uint32_t lazy_out) {
    uint64_t t_entry = 0;
    if constexpr (frame_of<L, R, ARITH>::TRACE) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_entry) : : "memory");
    if constexpr (frame_of<L, R, ARITH>::PRIO) __builtin_amdgcn_s_setprio(3);
    AGX_RB2_PROLOGUE;
    f.lazy_out = lazy_out != 0;
    uint64_t x[C];
    // kept old form: fwd_rb2 (every instance) -- through a load_pass0 member the slab address and the lazy_out test move ahead of the frame loads
    if constexpr (F::NT_LOAD) {
        const uint64_t* src = in + base;     // wave-uniform
#pragma unroll
        for (int r = 0; r < C; ++r) x[r] = __builtin_nontemporal_load(src + (uint32_t)r * T + f.tid);
    } else if constexpr (F::SCALAR_BASE) {
        const uint64_t* src = in + base;     // wave-uniform
#pragma unroll
        for (int r = 0; r < C; ++r) x[r] = (src + (uint32_t)r * T)[f.tid];
    } else {
#pragma unroll
        for (int r = 0; r < C; ++r) x[r] = in[base + f.tid + (uint32_t)r * T];
    }
    if constexpr (F::PRIO && !F::PRIO_BARRIER) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_setprio(0);
    }
    if constexpr (F::TRACE) {
        f.ts[0] = t_entry;
        f.template stamp<1>(x[C - 1]);
    }
    f.forward(x, tw_rb + (size_t)prime * pairs_per_prime);
    f.store_last_layout(x, out, base, live);
}

// Loop kernels of the inverse (n = 16384 / 32768): a resident grid (as many workgroups as the chip holds at once) walks over the
// frames.  A workgroup that transforms frame after frame issues the next frame's loads right behind the current frame's stores, so
// the store drain of one frame and the load latency of the next overlap -- with one or two workgroups per CU (the frame's image fills
// the LDS) nothing else on the CU could cover either.  The frame-to-frame hand-over of the LDS image needs one bare s_barrier.
// inv_rb2_dloop draws its frames from a ticket counter (a CU that runs a few per cent faster simply takes more frames): thread 0
// draws one frame ahead, right behind the frame loads, and hands the number round through a two-slot LDS mailbox that everybody reads
// behind the frame's own cross-wave barrier.  ticket[0] = frames handed out beyond the first round, ticket[1] = retired workgroups;
// the last workgroup out zeroes both (the plan keeps one pair per stream).  inv_rb2_loop walks with a fixed stride and carries no
// state: it serves launches that are being captured into a hipGraph and streams that have no pair (agx_ntt.cpp: plan_ticket_for).
// The forward transform measured slower in both forms (-3 ... -6 %, profiles/r03_streamed_kernels_sweeps.txt) and stays one
// workgroup per frame.
__device__ __forceinline__ void dloop_retire(uint32_t* ticket) {
    if (threadIdx.x == 0) {
        if (atomicAdd(ticket + 1, 1u) == gridDim.x - 1) {     // last workgroup out: reset the pair for its next launch
            __threadfence();
            ticket[0] = 0;
            ticket[1] = 0;
        }
    }
}

// kept old form: the per-frame body of inv_rb2, inv_rb2_loop and inv_rb2_dloop is spelled out in each -- as one shared function every instance is rescheduled
template <int L, int R, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)), MINW)
inv_rb2_dloop(const uint64_t* __restrict__ in, const uint64_t* __restrict__ in2, uint64_t* __restrict__ out,
              const prime_consts* __restrict__ consts, const twpair* __restrict__ itw_rb,
              uint32_t pairs_per_prime, uint32_t batch, uint32_t total, int64_t prime_stride, int64_t poly_stride,
              uint32_t* __restrict__ ticket) {
    using F = frame_of<L, R, ARITH>;
    static_assert(!F::G::exchange_is_wave_local(0), "the mailbox is read behind the last exchange's workgroup barrier");
    constexpr int C = F::C, T = F::T;
    F f;
    f.tid = threadIdx.x;
    f.slab = reinterpret_cast<uint64_t*>(agx_dyn_lds);
    volatile uint32_t* mailbox = reinterpret_cast<volatile uint32_t*>(reinterpret_cast<unsigned char*>(f.slab) + F::image_bytes);
    uint32_t fr = blockIdx.x;
    for (uint32_t it = 0;; ++it) {
        const uint32_t prime = fr / batch, poly = fr % batch;
        const int64_t base = (int64_t)prime * prime_stride + (int64_t)poly * poly_stride;
        const prime_consts pc = consts[prime];
        const barrett128 bk{pc.q, pc.mu_hi, pc.mu_lo};
        f.init_consts(pc.q, pc.est);
        uint64_t x[C];
        f.load_last_issue(x, in, base);
        if (threadIdx.x == 0) mailbox[it & 1u] = atomicAdd(ticket, 1u) + gridDim.x;
        if (it) __builtin_amdgcn_s_barrier();   // every wave has read the previous frame's last exchange
        f.load_last_stage(x, in2, bk, base);
        f.inverse(x, itw_rb + (size_t)prime * pairs_per_prime, pc);      // its last exchange is a workgroup barrier: the mailbox is visible behind it
        const uint32_t next = (uint32_t)__builtin_amdgcn_readfirstlane((int)mailbox[it & 1u]);
        // kept old form: inv_rb2_dloop<14, 5, kLazy, 4> -- through store_pass0 the stores are scheduled differently around the mailbox read
#pragma unroll
        for (int r = 0; r < C; ++r) {
            if constexpr (F::NT_STORE) __builtin_nontemporal_store(x[r], &out[base + f.tid + (uint32_t)r * T]);
            else out[base + f.tid + (uint32_t)r * T] = x[r];
        }
        fr = next;
        if (fr >= total) break;
    }
    dloop_retire(ticket);
}

template <int L, int R, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)), MINW)
inv_rb2_loop(const uint64_t* __restrict__ in, const uint64_t* __restrict__ in2, uint64_t* __restrict__ out,
             const prime_consts* __restrict__ consts, const twpair* __restrict__ itw_rb,
             uint32_t pairs_per_prime, uint32_t batch, uint32_t total, int64_t prime_stride, int64_t poly_stride) {
    using F = frame_of<L, R, ARITH>;
    constexpr int C = F::C;
    F f;
    f.tid = threadIdx.x;
    f.slab = reinterpret_cast<uint64_t*>(agx_dyn_lds);
    bool first = true;
    for (uint32_t fr = blockIdx.x; fr < total; fr += gridDim.x) {
        const uint32_t prime = fr / batch, poly = fr % batch;
        const int64_t base = (int64_t)prime * prime_stride + (int64_t)poly * poly_stride;
        const prime_consts pc = consts[prime];
        const barrett128 bk{pc.q, pc.mu_hi, pc.mu_lo};
        f.init_consts(pc.q, pc.est);
        uint64_t x[C];
        f.load_last_issue(x, in, base);
        // the previous frame's last exchange is read across waves: nobody may stage into the image before all have read
        if (!first) __builtin_amdgcn_s_barrier();
        f.load_last_stage(x, in2, bk, base);
        f.inverse(x, itw_rb + (size_t)prime * pairs_per_prime, pc);
        f.store_pass0(x, out, base);
        first = false;
    }
}

template <int L, int R, int PPB, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)) * PPB, MINW)
inv_rb2(const uint64_t* __restrict__ in, const uint64_t* __restrict__ in2, uint64_t* __restrict__ out,
        const prime_consts* __restrict__ consts, const twpair* __restrict__ itw_rb,
        uint32_t pairs_per_prime, uint64_t frames_x,
        int64_t prime_stride, int64_t poly_stride) {
    uint64_t t_entry = 0;
    if constexpr (frame_of<L, R, ARITH>::TRACE) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_entry) : : "memory");
    if constexpr (frame_of<L, R, ARITH>::PRIO) __builtin_amdgcn_s_setprio(3);   // until the frame loads are out
    AGX_RB2_PROLOGUE;
    const prime_consts pc = consts[prime];
    const barrett128 bk{pc.q, pc.mu_hi, pc.mu_lo};
    uint64_t x[C];
    f.load_last_issue(x, in, base);
    if constexpr (F::TRACE) {
        f.ts[0] = t_entry;
        f.template stamp<1>(x[C - 1]);      // frame arrived
    }
    f.load_last_stage(x, in2, bk, base);
    if constexpr (F::TRACE) f.template stamp<2>(x[C - 1]);      // staged through the image into the last pass's layout
    f.inverse(x, itw_rb + (size_t)prime * pairs_per_prime, pc);
    f.store_pass0(x, out, base, live);
    if constexpr (F::TRACE) {
        f.template stamp<10>(x[0]);         // stores issued
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        f.template stamp<11>(x[0]);         // stores retired
        f.trace_flush();
    }
}

// c = INTT(NTT(a) o NTT(b)) for one frame without leaving the chip: both forward transforms end in
// the same register layout, the product is taken there, and the inverse starts from it (no staging
// through the image at either seam).  HBM traffic 24n bytes per product.
template <int L, int R, int PPB, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)) * PPB, (MINW > AGX_POLYMUL_MAXW ? AGX_POLYMUL_MAXW : MINW))   // one frame more in registers
polymul_rb2(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, uint64_t* __restrict__ c,
            const prime_consts* __restrict__ consts, const twpair* __restrict__ tw_rb, const twpair* __restrict__ itw_rb,
            uint32_t pairs_per_prime, uint64_t frames_x, int64_t prime_stride, int64_t poly_stride) {
    AGX_RB2_PROLOGUE;
    const prime_consts pc = consts[prime];
    const barrett128 bk{pc.q, pc.mu_hi, pc.mu_lo};
    // q <= 2^60: the product below takes operands in [0,4q) (16 q^2 < 2^124, quotient < 16q <= 2^64), so
    // both forward transforms may skip their last two conditional subtracts
    f.lazy_out = F::LAZY16;
    uint64_t xa[C], xb[C];
    // kept old form (both loads): polymul_rb2<12, 3, 1, ...> -- through load_pass0 the slab address moves ahead of the frame loads
    constexpr bool NTL = F::NT_LOAD;
#pragma unroll
    for (int r = 0; r < C; ++r) xa[r] = NTL ? __builtin_nontemporal_load(&a[base + f.tid + (uint32_t)r * T]) : a[base + f.tid + (uint32_t)r * T];
    f.forward(xa, tw_rb + (size_t)prime * pairs_per_prime);
    // b is fetched only now: holding it across NTT(a) would cost 2^R more register pairs and spill
#pragma unroll
    for (int r = 0; r < C; ++r) xb[r] = NTL ? __builtin_nontemporal_load(&b[base + f.tid + (uint32_t)r * T]) : b[base + f.tid + (uint32_t)r * T];
    __syncthreads();   // the image is reused: every wave must be done reading NTT(a)'s exchanges
    f.forward(xb, tw_rb + (size_t)prime * pairs_per_prime);
#pragma unroll
    for (int r = 0; r < C; ++r) xa[r] = mul_mod_barrett(xa[r], xb[r], bk);
    f.inverse(xa, itw_rb + (size_t)prime * pairs_per_prime, pc);
    f.store_pass0(xa, c, base, live);
}

// The same product with only ONE frame in registers at a time: NTT(first) is parked in c's own frame (plain global
// memory: written, and read back a few microseconds later by the same workgroup, so it is served by the XCD's L2)
// while NTT(second) is computed, then fetched in the last pass's layout (each thread its 2^R consecutive
// coefficients), multiplied, and the inverse starts from there.  This is what lets n = 16384 (16 coefficients per
// thread: two frames do not fit 128 VGPRs) run the product in one launch, and what frees the smaller sizes from the
// second frame's registers.  The host passes as `first` the operand c aliases, if any: a workgroup reads all of
// `first` before it writes c, and `second` is then a different buffer.  Squaring (a == b, with or without c aliasing
// them) never comes here: `second` would be the parked words themselves when c aliases too, so the
// launcher sends it to polysquare_rb2 below (a branch on first == second inside this kernel cost 240-320 B of scratch).
template <int L, int R, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)), MINW)
polymul_rb2_park(const uint64_t* __restrict__ first, const uint64_t* __restrict__ second, uint64_t* __restrict__ c,
                 const prime_consts* __restrict__ consts, const twpair* __restrict__ tw_rb, const twpair* __restrict__ itw_rb,
                 uint32_t pairs_per_prime, uint64_t frames_x, int64_t prime_stride, int64_t poly_stride) {
    constexpr int PPB = 1;
    AGX_RB2_PROLOGUE;
    const prime_consts pc = consts[prime];
    const barrett128 bk{pc.q, pc.mu_hi, pc.mu_lo};
    f.lazy_out = F::LAZY16;     // the Barrett product takes operands in [0,4q) when q <= 2^60
    uint64_t x[C];
    f.load_pass0(x, first, base);
    f.forward(x, tw_rb + (size_t)prime * pairs_per_prime);
    static_assert(F::STREAM_TW, "the parked product is a streamed single-frame kernel");
    {
        // Thread-private parking: every thread stores its own 2^R values of NTT(first) (register r at c[base + tid + r T]: lane-contiguous,
        // not the natural element order -- c's frame is only scratch here) and later reads back exactly the words it wrote, one
        // register at a time, so the product needs neither an LDS redistribution nor a second frame in registers.
        if (live) {
#pragma unroll
            for (int r = 0; r < C; ++r) c[base + f.tid + (uint32_t)r * T] = x[r];
        }
        asm volatile("" ::: "memory");      // the second operand's loads stay behind the parking stores (or two frames would be live)
        __builtin_amdgcn_sched_barrier(0);
        f.load_pass0(x, second, base);
        __syncthreads();   // the image is reused
        {
            const twpair* tbl2 = tw_rb + (size_t)prime * pairs_per_prime;
            asm volatile("" : "+s"(tbl2));      // opaque: or the first transform's table entries are kept (spilled) for reuse instead of re-read from L2
            f.forward(x, tbl2);
        }
        const uint64_t* parked = c;
        asm volatile("" : "+s"(parked));      // opaque: the compiler must re-load the parked words, not keep them in registers
        constexpr int GRP = 4;
        static_for<0, C / GRP>([&](auto Gq) {
            constexpr int g = Gq;
            uint64_t z[GRP];
            static_for<0, GRP>([&](auto I) { constexpr int r = g * GRP + (int)I; z[I] = parked[base + f.tid + (uint32_t)r * T]; });
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, GRP>([&](auto I) {
                constexpr int r = g * GRP + (int)I;
                asm volatile("" : "+v"(x[r]));
                x[r] = mul_mod_barrett(z[I], x[r], bk);
                asm volatile("" : "+v"(x[r]));
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        f.inverse(x, itw_rb + (size_t)prime * pairs_per_prime, pc);
        f.store_pass0(x, c, base, live);
    }
}

// c = a * a in Z_q[X]/(X^n + 1): one forward transform, the product of every coefficient with itself where it sits in
// registers, the inverse.  16n bytes of traffic; a workgroup reads its whole frame before it writes any of it, so c may
// alias a.  Serves agx_ntt_polymul calls with a == b on the plans whose fused product is polymul_rb2_park.
template <int L, int R, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)), MINW)
polysquare_rb2(const uint64_t* __restrict__ a, uint64_t* __restrict__ c,
               const prime_consts* __restrict__ consts, const twpair* __restrict__ tw_rb, const twpair* __restrict__ itw_rb,
               uint32_t pairs_per_prime, uint64_t frames_x, int64_t prime_stride, int64_t poly_stride) {
    constexpr int PPB = 1;
    AGX_RB2_PROLOGUE;
    const prime_consts pc = consts[prime];
    const barrett128 bk{pc.q, pc.mu_hi, pc.mu_lo};
    f.lazy_out = F::LAZY16;     // the Barrett product takes operands in [0,4q) when q <= 2^60
    uint64_t x[C];
    // kept old form: polysquare_rb2<12, 5, kLazy | kOptPrio, 4> (diagnostics twin) -- through load_pass0 its loads are scheduled differently
#pragma unroll
    for (int r = 0; r < C; ++r) x[r] = F::NT_LOAD ? __builtin_nontemporal_load(&a[base + f.tid + (uint32_t)r * T]) : a[base + f.tid + (uint32_t)r * T];
    f.forward(x, tw_rb + (size_t)prime * pairs_per_prime);
#pragma unroll
    for (int r = 0; r < C; ++r) {
        asm volatile("" : "+v"(x[r]));
        x[r] = mul_mod_barrett(x[r], x[r], bk);
        asm volatile("" : "+v"(x[r]));
    }
    __syncthreads();   // the image is reused: every wave is done reading the forward transform's exchanges
    f.inverse(x, itw_rb + (size_t)prime * pairs_per_prime, pc);
    f.store_pass0(x, c, base, live);
}

// c = a * b in Z_q[X]/(X^n + 1) with b given by its transform bhat (what agx_ntt_forward / agx_ntt_forward_lazy of this plan wrote:
// bit-reversed order, so thread tid's registers 0 .. C-1 of the last pass's layout meet bhat words tid C .. tid C + C-1): one forward
// transform, the product where the coefficients sit in registers, the inverse.  One frame in registers at any time; nothing is
// parked.  bhat has strides of its own: a poly stride of 0 multiplies every frame of a prime by the same bhat frame.  Each lane
// reads its own C consecutive words of bhat with 16-byte loads (plain loads: a shared bhat should stay in L2 / MALL), GRP registers'
// worth at a time and one group ahead of the one being multiplied; the kernels that run the forward transform pass by pass
// (no streamed twiddles) request the first groups before the last forward pass.  24n bytes of traffic per product with a bhat frame per
// frame, 16n + 8n / batch with a shared one.  A workgroup reads its whole frame of a before it writes c: c may alias a.
typedef uint64_t bhat_pair __attribute__((ext_vector_type(2), aligned(8)));      // bhat is only known to be 8-byte aligned

template <int L, int R, int PPB, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)) * PPB, (MINW > AGX_MULHAT_MAXW ? AGX_MULHAT_MAXW : MINW))
mulhat_rb2(const uint64_t* __restrict__ a, const uint64_t* __restrict__ bhat, uint64_t* __restrict__ c,
           const prime_consts* __restrict__ consts, const twpair* __restrict__ tw_rb, const twpair* __restrict__ itw_rb,
           uint32_t pairs_per_prime, uint64_t frames_x, int64_t prime_stride, int64_t poly_stride,
           int64_t bhat_prime_stride, int64_t bhat_poly_stride) {
    AGX_RB2_PROLOGUE;
    const prime_consts pc = consts[prime];
    const barrett128 bk{pc.q, pc.mu_hi, pc.mu_lo};
    f.lazy_out = F::LAZY16;     // the Barrett product takes operands in [0,4q) when q <= 2^60
    constexpr bool NTL = F::NT_LOAD;
    constexpr int GRP = 4, NG = C / GRP;      // registers per group of bhat loads (two 16-byte loads), groups per thread
    static_assert(C % GRP == 0, "whole groups");
    // pass by pass forward kernels (R = 3, 8 waves/SIMD, 16 words of bhat per thread): every group is requested before the last
    // forward pass; streamed kernels (R = 4 / 5: the whole transform is one call) request group g + 1 before they multiply group g
    constexpr bool EARLY = !F::STREAM_TW && !F::SPLIT && F::NP >= 2 && NG <= 2;
    const bhat_pair* bp = reinterpret_cast<const bhat_pair*>(bhat + ((int64_t)prime * bhat_prime_stride + (int64_t)fx * bhat_poly_stride) + (uint32_t)f.tid * C);
    uint64_t x[C];
    // kept old form: mulhat_rb2 (every instance) -- through load_pass0 the slab address moves ahead of the frame loads
#pragma unroll
    for (int r = 0; r < C; ++r) x[r] = NTL ? __builtin_nontemporal_load(&a[base + f.tid + (uint32_t)r * T]) : a[base + f.tid + (uint32_t)r * T];
    bhat_pair z[EARLY ? NG : 2][GRP / 2];
    auto request = [&](auto Gq) {
        constexpr int g = Gq;
        static_for<0, GRP / 2>([&](auto I) { z[EARLY ? g : (g & 1)][I] = bp[g * (GRP / 2) + (int)I]; });
    };
    if constexpr (EARLY) {
        f.template forward_passes<0, F::NP - 1>(x, tw_rb + (size_t)prime * pairs_per_prime);
        static_for<0, NG>(request);
        f.template forward_passes<F::NP - 1, F::NP>(x, tw_rb + (size_t)prime * pairs_per_prime);
    } else {
        f.forward(x, tw_rb + (size_t)prime * pairs_per_prime);
        request(std::integral_constant<int, 0>{});
    }
    static_for<0, NG>([&](auto Gq) {
        constexpr int g = Gq;
        if constexpr (!EARLY && g + 1 < NG) request(std::integral_constant<int, g + 1>{});
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, GRP>([&](auto I) {
            constexpr int i = I, r = g * GRP + i;
            uint64_t u = z[EARLY ? g : (g & 1)][i / 2][i & 1];
            // forward_lazy may have left bhat in [0,4q); beyond 2^60 the product wants it (and NTT(a), which is then fully reduced) below q
            if constexpr (!F::LAZY16) u = reduce_4q(u, pc.q, pc.q << 1);
            asm volatile("" : "+v"(x[r]));
            x[r] = mul_mod_barrett(x[r], u, bk);
            asm volatile("" : "+v"(x[r]));
        });
        __builtin_amdgcn_sched_barrier(0);
    });
    __syncthreads();   // the image is reused: every wave is done reading the forward transform's exchanges
    f.inverse(x, itw_rb + (size_t)prime * pairs_per_prime, pc);
    f.store_pass0(x, c, base, live);
}

// The second launch of agx_ntt_rescale (exact division by the last RNS modulus q_L on NTT-form frames) for primes i < P-1:
// out_i = (x_i - NTT_i(u_i)) q_L^-1 mod q_i, u_i = the lift of t to q_i (rescale_lift, modarith.hpp), t = INTT_L(x_L) in [0,q_L) as the
// first launch (the plan's inverse on the view of prime P-1) left it in the scratch: dense [batch][n], read by the P-1 workgroups of
// a frame (plain loads: it should stay in L2).  The frame of t is loaded in the pass-0 layout and lifted where it sits in registers,
// then transformed; in the last pass's layout every lane streams in its own C consecutive words of x_i (16-byte loads, requested
// ahead exactly as mulhat_rb2 requests bhat), which may be lazy ([0,4q), as agx_ntt_forward_lazy leaves them), and the result leaves
// through the forward kernels' store.  One frame in registers; 16n bytes per (prime, frame) plus 8n per frame for t.
// out may BE x (in place): a wave stores exactly the 64 C contiguous words its own lanes loaded from x (the last pass is
// wave-contiguous), and store_last_layout relays them through the image behind a wavefront-scope release / acquire pair, which keeps
// every load of x ahead of every store of the wave.  x and out are therefore not __restrict__.  Slots of a partly filled workgroup
// read the last frame again and store nothing.
template <int L, int R, int PPB, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)) * PPB, (MINW > AGX_MULHAT_MAXW ? AGX_MULHAT_MAXW : MINW))
rescale_rb2(const uint64_t* x, const uint64_t* __restrict__ t, uint64_t* out,
            const prime_consts* __restrict__ consts, const rescale_consts* __restrict__ rcs, const twpair* __restrict__ tw_rb,
            uint32_t pairs_per_prime, uint64_t frames_x, int64_t prime_stride, int64_t poly_stride, uint32_t round) {
    AGX_RB2_PROLOGUE;
    const prime_consts pc = consts[prime];
    const rescale_consts rc = rcs[prime];
    const barrett128 bk{pc.q, pc.mu_hi, pc.mu_lo};
    const uint64_t h = round ? rc.h : 0, hq = round ? rc.h_mod_q : 0;      // wave-uniform
    // q <= 2^60: rescale_finish takes both operands in [0,4q), so the transform may skip its last conditional subtracts and x_i needs no reduction
    f.lazy_out = F::LAZY16;
    constexpr int GRP = 4, NG = C / GRP;      // registers per group of x loads (two 16-byte loads), groups per thread
    static_assert(C % GRP == 0, "whole groups");
    constexpr bool EARLY = !F::STREAM_TW && !F::SPLIT && F::NP >= 2 && NG <= 2;      // as mulhat_rb2
    const bhat_pair* xp = reinterpret_cast<const bhat_pair*>(x + base + (uint32_t)f.tid * C);
    uint64_t u[C];
    const uint64_t* tf = t + (int64_t)fx * poly_stride;      // input prime stride 0: every prime of the frame reads the same words
#pragma unroll
    for (int r = 0; r < C; ++r) u[r] = tf[f.tid + (uint32_t)r * T];
#pragma unroll
    for (int r = 0; r < C; ++r) u[r] = rescale_lift(u[r], h, hq, rc.q_last, bk);      // [0,q_L) -> [0,q)
    bhat_pair z[EARLY ? NG : 2][GRP / 2];
    auto request = [&](auto Gq) {
        constexpr int g = Gq;
        static_for<0, GRP / 2>([&](auto I) { z[EARLY ? g : (g & 1)][I] = xp[g * (GRP / 2) + (int)I]; });
    };
    if constexpr (EARLY) {
        f.template forward_passes<0, F::NP - 1>(u, tw_rb + (size_t)prime * pairs_per_prime);
        static_for<0, NG>(request);
        f.template forward_passes<F::NP - 1, F::NP>(u, tw_rb + (size_t)prime * pairs_per_prime);
    } else {
        f.forward(u, tw_rb + (size_t)prime * pairs_per_prime);
        request(std::integral_constant<int, 0>{});
    }
    static_for<0, NG>([&](auto Gq) {
        constexpr int g = Gq;
        if constexpr (!EARLY && g + 1 < NG) request(std::integral_constant<int, g + 1>{});
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, GRP>([&](auto I) {
            constexpr int i = I, r = g * GRP + i;
            uint64_t v = z[EARLY ? g : (g & 1)][i / 2][i & 1];
            // beyond 2^60 the difference wants x_i (lazy: below 4q, which may not fit 64 bits -- reduce_4q never forms it) and NTT(u), which is then
            // fully reduced, below q
            if constexpr (!F::LAZY16) v = reduce_4q(v, pc.q, pc.q << 1);
            asm volatile("" : "+v"(u[r]));
            u[r] = rescale_finish<F::LAZY16>(v, u[r], rc.qlinv, rc.qlinv_p, pc.q);
            asm volatile("" : "+v"(u[r]));
        });
        __builtin_amdgcn_sched_barrier(0);
    });
    f.store_last_layout(u, out, base, live);
}

// agx_ntt_basis_extend to NTT form in one launch: fast RNS base conversion from the S source primes of a basis to ONE target prime, then that
// prime's forward transform, one frame on chip.  x: dense [S][batch][n] in coefficient form (slab i under plan prime src_first + i, values in
// [0,4q_i)); out: dense [T][batch][n], slab j under plan prime dst_first + j, written exactly as fwd_rb2 writes it.  For each source the
// frame's words arrive in the pass-0 layout, GRP registers at a time and one group ahead of the one being folded in (plain loads: the T
// workgroups of a frame all read them); y_i = x_i D_i^-1 mod q_i is formed in [0,q_i) and y_i (D_i mod q_j) is
// added to the frame's accumulators, which stay in [0,2q_j) (basis_accumulate, modarith.hpp): one 64-bit accumulator per coefficient, so
// the frame, one group in flight and one being folded are all that is live.  The forward passes take [0,2q_j) as it is.  Each workgroup
// forms the y_i of its frame again, so a workgroup does 2 S Shoup products per output word (S to form the y_i, S to fold them in) beside the
// log2(n) / 2 butterflies per word of the transform: at S = 16 that is 32 against 5 ... 7.5, and the host routes by S (extend_is_fused, agx_ntt.cpp).
// BLOCK ORDER: the linear block index has the TARGET PRIME FASTEST, so the T workgroups of a group of frames are dispatched together (with the
// prime on blockIdx.y, AGX_RB2_PROLOGUE, every frame of target 0 would run before any of target 1).  Measured, this does not make them share
// the sources in L2: the L2s request about T times the source bytes (profiles/r08_basis_extend.md).
template <int L, int R, int PPB, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)) * PPB, (MINW > AGX_MULHAT_MAXW ? AGX_MULHAT_MAXW : MINW))
extend_rb2(const uint64_t* __restrict__ x, uint64_t* __restrict__ out, const prime_consts* __restrict__ consts, const ulonglong2* __restrict__ dinv,
           const ulonglong2* __restrict__ mat, const twpair* __restrict__ tw_rb, uint32_t pairs_per_prime, uint64_t frames_x,
           int64_t prime_stride, int64_t poly_stride, uint32_t src_first, uint32_t num_src, uint32_t dst_first, uint32_t num_dst) {
    using F = frame_of<L, R, ARITH>;
    constexpr int C = F::C, T = F::T;
    static_assert(T >= 64, "one frame must span whole waves");
    F f;
    f.tid = threadIdx.x & (T - 1);
    const uint32_t slot = PPB == 1 ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / T));      // a frame spans whole waves: wave-uniform
    // the quotient comes out of the vector unit (there is no scalar divide): pin it to a scalar register, or every address derived from it is
    // held in vector registers for the whole kernel (R = 5: 12 ... 20 bytes of scratch per lane)
    uint32_t group = blockIdx.x / num_dst;
    asm volatile("" : "+s"(group));
    const uint32_t j = blockIdx.x - group * num_dst;
    uint64_t fx = (uint64_t)group * PPB + slot;
    const bool live = fx < frames_x;
    if (!live) fx = frames_x - 1;                         // keep every thread on the barriers
    const uint32_t prime = dst_first + j;
    const uint64_t q = consts[prime].q, q2 = q << 1;
    f.init_consts(q, consts[prime].est);
    f.slab = reinterpret_cast<uint64_t*>(agx_dyn_lds) + (size_t)slot * F::slab_elems;
    int64_t base = (int64_t)j * prime_stride + (int64_t)fx * poly_stride;
    constexpr int GRP = 4, NG = C / GRP;      // registers per group of source loads, groups per thread
    static_assert(C % GRP == 0 && NG % 2 == 0, "whole groups, and group 0 of every source in buffer 0");
    const uint64_t* xf = x + (int64_t)fx * poly_stride;      // the frame under source 0 (wave-uniform: lanes add tid)
    // both wave-uniform and pinned to scalar registers of their own: sharing fx poly_stride, they were kept as one vector pair to the last store
    asm volatile("" : "+s"(base), "+s"(xf));
    const ulonglong2* row = mat + (size_t)j * num_src;
    uint64_t acc[C], z[2][GRP];
#pragma unroll
    for (int r = 0; r < C; ++r) acc[r] = 0;
    static_for<0, GRP>([&](auto I) { z[0][I] = xf[f.tid + (uint32_t)(int)I * T]; });
    for (uint32_t i = 0; i < num_src; ++i) {      // wave-uniform
        const uint64_t qi = consts[src_first + i].q;
        const ulonglong2 d = dinv[i], c = row[i];
        const uint64_t* cur = xf + (int64_t)i * prime_stride;
        const uint64_t* nxt = xf + (int64_t)(i + 1 < num_src ? i + 1 : i) * prime_stride;      // behind the last source: its own first group again (a cache hit, dropped)
        static_for<0, NG>([&](auto Gq) {
            constexpr int g = Gq;
            // the group's first word, opaque and scalar: every group then shares the GRP lane offsets tid + I T.  Seen through, the C distinct
            // offsets r T (beyond the instruction's immediate from T = 512 on) are hoisted out of this loop into C register pairs, which spill
            const uint64_t* pg = g + 1 < NG ? cur + (uint32_t)((g + 1) * GRP) * T : nxt;
            asm volatile("" : "+s"(pg));
            static_for<0, GRP>([&](auto I) { z[(g + 1) & 1][I] = pg[f.tid + (uint32_t)(int)I * T]; });
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, GRP>([&](auto I) {
                constexpr int r = g * GRP + (int)I;
                asm volatile("" : "+v"(acc[r]));
                acc[r] = basis_accumulate(acc[r], basis_scale(z[g & 1][I], d.x, d.y, qi), c.x, c.y, q, q2);
                asm volatile("" : "+v"(acc[r]));
            });
            __builtin_amdgcn_sched_barrier(0);
        });
    }
    f.forward(acc, tw_rb + (size_t)prime * pairs_per_prime);
    f.store_last_layout(acc, out, base, live);
}

// The second launch of agx_ntt_basis_mod_down (ModDown of a hybrid key switch on NTT-form frames) for ONE target prime j of a basis:
// out_j = (xq_j - NTT_j(sum_i y_i (D_i mod q_j))) D^-1 mod q_j, one frame on chip.  y: dense [S][batch][n], y_i = p_i D_i^-1 mod q_i in [0,q_i) as
// the first launch left it in the scratch -- the plan's inverse on the source slabs with n^-1 D_i^-1 for n^-1 -- so there is no basis_scale here:
// S Shoup products per output word, where extend_rb2 does 2 S.  The accumulation is extend_rb2's: the frame's words of every source arrive in the
// pass-0 layout, GRP registers at a time and one group ahead of the one being folded in (plain loads: the T workgroups of a frame all read them),
// one 64-bit accumulator per coefficient in [0,2q_j), which the forward passes take as it is.  The finish is rescale_rb2's: in the last pass's
// layout every lane streams in its own C consecutive words of xq_j (16-byte loads requested ahead; lazy values allowed) and forms
// (xq_j - acc) D^-1 mod q_j (rescale_finish: the lazy form for q <= 2^60, reduce_4q first otherwise), and the result leaves through the forward
// kernels' store.  8n(S + 2) bytes per (target, frame) as requested by the workgroup.
// out may BE xq (in place), by rescale_rb2's argument: a wave stores exactly the 64 C contiguous words its own lanes loaded from xq, and
// store_last_layout relays them through the image behind a wavefront-scope release / acquire pair.  xq and out are therefore not __restrict__.
// Block order and the three pinned scalars (group, base, yf) as in extend_rb2.
// AGX_RESCALE_ROUND (agx_ntt_basis_mod_down_mode) is the same text with the two per-word steps of moddown_arith.hpp: every y_i gets c_i = rsrc[i].x added
// modulo q_i = rsrc[i].y as it streams in, and hq_j = rdst[j] leaves the accumulators, which stay in [0,2q_j), before the forward passes: S + 1
// add-and-conditional-subtract pairs per word.  The body is written once, in moddown_rb2_body.hpp, and included in its two kernels: moddown_rb2 (FLOOR:
// what it always was, rsrc and rdst never read) and moddown_round_rb2.  A plaintext modulus t is in the constants alone (mat = t D_i mod q_j, the scaled
// inverse's t^-1).
template <int L, int R, int PPB, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)) * PPB, (MINW > AGX_MULHAT_MAXW ? AGX_MULHAT_MAXW : MINW))
moddown_rb2(const uint64_t* xq, const uint64_t* __restrict__ y, uint64_t* out, const prime_consts* __restrict__ consts, const ulonglong2* __restrict__ mat,
            const ulonglong2* __restrict__ dall, const twpair* __restrict__ tw_rb, uint32_t pairs_per_prime, uint64_t frames_x, int64_t prime_stride,
            int64_t poly_stride, uint32_t num_src, uint32_t dst_first, uint32_t num_dst) {
    [[maybe_unused]] constexpr bool ROUND = false;
    [[maybe_unused]] constexpr const ulonglong2* rsrc = nullptr;
    [[maybe_unused]] constexpr const uint64_t* rdst = nullptr;
#include "moddown_rb2_body.hpp"
}

// rsrc: [S] {c_i = h D_i^-1 mod q_i, q_i}; rdst: [T] t h mod q_j (agx_ntt_basis: d_round_src, d_round_dst)
template <int L, int R, int PPB, int ARITH, int MINW>
__global__ void __launch_bounds__((1 << (L - R)) * PPB, (MINW > AGX_MULHAT_MAXW ? AGX_MULHAT_MAXW : MINW))
moddown_round_rb2(const uint64_t* xq, const uint64_t* __restrict__ y, uint64_t* out, const prime_consts* __restrict__ consts, const ulonglong2* __restrict__ mat,
                  const ulonglong2* __restrict__ dall, const twpair* __restrict__ tw_rb, uint32_t pairs_per_prime, uint64_t frames_x, int64_t prime_stride,
                  int64_t poly_stride, uint32_t num_src, uint32_t dst_first, uint32_t num_dst, const ulonglong2* __restrict__ rsrc,
                  const uint64_t* __restrict__ rdst) {
    [[maybe_unused]] constexpr bool ROUND = true;
#include "moddown_rb2_body.hpp"
}

// ---- host side: pass tables, launch glue and registry entries, written once for every kernel family ---------------------------------
// (the 32-bit kernels of rb32_kernels.hpp and the wave-packed kernels of wp_kernels.hpp bring their own shape struct and nothing else)

// The geometry of one prime's pass table: f(at, idx) for every slot `at` in [0, rb_geom<L, R>::table_pairs) that holds a twiddle, idx = its
// natural twiddle index.  What a slot stores is the builder's business ({w, w'} in build_table_t, the two split twiddles in build_table_fold_t,
// {(u32)w, w' >> 32} in build_table32_t); rb_entry::build hands every builder the prime's modulus.
template <int L, int R, class F>
void for_each_table_slot(F&& f) {
    using G = rb2_geom<L, R>;
    for (int p = 0; p < G::NP; ++p) {
        const int rlo = G::rlo(p), hi = G::hi(p), H = G::H(p);
        for (int j = 1; j < G::C; ++j) {
            int k = 0;
            while ((2 << k) <= j) ++k;
            const int o = j - (1 << k), rb_bit = R - 1 - k, b = rlo + rb_bit;
            if (b > hi) continue;  // stage belongs to an earlier pass (short last pass)
            const uint32_t m_local = 1u << (L - 1 - b);
            for (int h = 0; h < H; ++h) {
                const uint32_t idx = m_local + ((uint32_t)h << k) + (uint32_t)o;      // natural twiddle index m + i (ntt.cpp:298-300)
                // wave-uniform passes keep one column's C entries contiguous (wide scalar loads);
                // per-lane passes keep one entry's columns contiguous (coalesced vector loads)
                const size_t at = G::uniform_pass(p) ? (size_t)h * G::C + j : (size_t)j * H + h;
                f((size_t)G::table_off(p) + at, idx);
            }
        }
    }
}

template <int L, int R>
void build_table_t(const uint64_t* tw, const uint64_t* pre, uint64_t, std::vector<ulonglong2>& out) {
    const size_t start = out.size();
    out.resize(start + (size_t)rb_geom<L, R>::table_pairs, make_ulonglong2(0, 0));
    for_each_table_slot<L, R>([&](size_t at, uint32_t idx) { out[start + at] = make_ulonglong2(tw[idx], pre[idx]); });
}
// the same geometry for the kernels of the two-twiddle butterfly (kOptQ60cFold): a slot holds fold_twiddle_pack(w, q), made from w alone
template <int L, int R>
void build_table_fold_t(const uint64_t* tw, const uint64_t*, uint64_t q, std::vector<ulonglong2>& out) {
    const size_t start = out.size();
    out.resize(start + (size_t)rb_geom<L, R>::table_pairs, make_ulonglong2(0, 0));
    for_each_table_slot<L, R>([&](size_t at, uint32_t idx) {
        const fold_twiddle f = fold_twiddle_pack(tw[idx], q);
        out[start + at] = make_ulonglong2(f.w_packed, f.wc_packed);
    });
}

template <class F>
constexpr int rb2_arith_level() { return F::Q60C ? 3 : F::LAZY16 ? 2 : F::FAST_ARITH ? 1 : 0; }      // rb_entry::arith

// A kernel shape S says what the launches of one family differ in besides the kernel symbol: the rb_entry fields (log_n, r, fpb = frames per
// workgroup, min_waves, table_pairs, lds, build, arith, narrow), threads per workgroup, and the flag word.  Every forward kernel ends in one:
// lazy_out here and in the wave-packed kernels (fwd_rb2 tests lazy_out != 0: it must never see another bit), q32_shape::flags in rb32_kernels.hpp,
// whose inverse and product kernels take one too (flags_everywhere).
struct lazy_flag {
    static constexpr bool flags_everywhere = false;
    static uint32_t flags(const void*, const void*, const void*, const frame_layout& fl) { return fl.lazy_out ? 1u : 0u; }
};

template <int L, int R, int PPB, int ARITH, int MINW>
struct rb2_shape : lazy_flag {
    static constexpr int log_n = L, r = R, fpb = PPB, threads = rb_geom<L, R>::T * PPB, min_waves = MINW, arith = rb2_arith_level<frame_of<L, R, ARITH>>(), narrow = 0;
    static constexpr uint32_t table_pairs = rb_geom<L, R>::table_pairs;
    static constexpr size_t lds = (size_t)frame_of<L, R, ARITH>::image_bytes * PPB;
    static constexpr auto build = frame_of<L, R, ARITH>::Q60C_FOLD ? &build_table_fold_t<L, R> : &build_table_t<L, R>;
};

// the one place the registry kernels' dynamic LDS is allowed: BYTES on each of K
template <size_t BYTES, auto... K>
hipError_t allow_lds() {
    hipError_t e = hipSuccess;
    ((e = e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BYTES)), ...);
    return e;
}

// one workgroup per S::fpb frames and prime
template <class S, class K, class... A>
hipError_t launch_frames(K kernel, const plan_view& pv, const frame_layout& fl, hipStream_t s, A... args) {
    const dim3 grid((unsigned)((fl.batch + S::fpb - 1) / S::fpb), pv.num_primes);
    hipLaunchKernelGGL(kernel, grid, dim3(S::threads), S::lds, s, args...);
    return hipGetLastError();
}

template <class S, auto K>
hipError_t launch_fwd_t(const plan_view& pv, const uint64_t* in, uint64_t* out, const frame_layout& fl, hipStream_t s) {
    return launch_frames<S>(K, pv, fl, s, in, out, pv.consts, pv.tw_rb, pv.rb->table_pairs, fl.batch, fl.prime_stride, fl.poly_stride,
                            S::flags(in, out, nullptr, fl));
}

template <class S, auto K>
hipError_t launch_inv_t(const plan_view& pv, const uint64_t* in, const uint64_t* in2, uint64_t* out, const frame_layout& fl, hipStream_t s) {
    if constexpr (S::flags_everywhere)
        return launch_frames<S>(K, pv, fl, s, in, in2, out, pv.consts, pv.itw_rb, pv.rb->table_pairs, fl.batch, fl.prime_stride, fl.poly_stride,
                                S::flags(in, in2, out, fl));
    else
        return launch_frames<S>(K, pv, fl, s, in, in2, out, pv.consts, pv.itw_rb, pv.rb->table_pairs, fl.batch, fl.prime_stride, fl.poly_stride);
}

template <class S, auto K>
hipError_t launch_mul_t(const plan_view& pv, const uint64_t* a, const uint64_t* b, uint64_t* c, const frame_layout& fl, hipStream_t s) {
    if constexpr (S::flags_everywhere)      // the product kernels read no flag
        return launch_frames<S>(K, pv, fl, s, a, b, c, pv.consts, pv.tw_rb, pv.itw_rb, pv.rb->table_pairs, fl.batch, fl.prime_stride, fl.poly_stride, 0u);
    else
        return launch_frames<S>(K, pv, fl, s, a, b, c, pv.consts, pv.tw_rb, pv.itw_rb, pv.rb->table_pairs, fl.batch, fl.prime_stride, fl.poly_stride);
}

// the product by a pre-transformed operand: the frame layout describes a and c, bhat brings its own two strides
template <class S, auto K>
hipError_t launch_mulhat_t(const plan_view& pv, const uint64_t* a, const uint64_t* bhat, uint64_t* c, const frame_layout& fl, int64_t bhat_prime_stride,
                           int64_t bhat_poly_stride, hipStream_t s) {
    return launch_frames<S>(K, pv, fl, s, a, bhat, c, pv.consts, pv.tw_rb, pv.itw_rb, pv.rb->table_pairs, fl.batch, fl.prime_stride, fl.poly_stride,
                            bhat_prime_stride, bhat_poly_stride);
}

// agx_ntt_rescale's second launch: pv is the view of primes 0 .. P-2, the frame layout describes x and out, t is dense [batch][n]
template <class S, auto K>
hipError_t launch_rescale_t(const plan_view& pv, const uint64_t* x, const uint64_t* t, uint64_t* out, const frame_layout& fl, bool round, hipStream_t s) {
    return launch_frames<S>(K, pv, fl, s, x, t, out, pv.consts, pv.rescale, pv.tw_rb, pv.rb->table_pairs, fl.batch, fl.prime_stride, fl.poly_stride,
                            round ? 1u : 0u);
}

// agx_ntt_basis_extend's fused launch: pv is the view of the whole plan, the frame layout describes x and out alike (dense); a linear grid, the
// target prime fastest (extend_rb2)
template <class S, auto K>
hipError_t launch_extend_t(const plan_view& pv, const basis_view& bv, const uint64_t* x, uint64_t* out, const frame_layout& fl, hipStream_t s) {
    const uint64_t blocks = (uint64_t)bv.dst_count * ((fl.batch + S::fpb - 1) / S::fpb);
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(K, dim3((unsigned)blocks), dim3(S::threads), S::lds, s, x, out, pv.consts, bv.dinv, bv.mat, pv.tw_rb, pv.rb->table_pairs, fl.batch,
                       fl.prime_stride, fl.poly_stride, bv.src_first, bv.src_count, bv.dst_first, bv.dst_count);
    return hipGetLastError();
}

// agx_ntt_basis_mod_down's second launch: pv is the view of the whole plan, the frame layout describes xq, y and out alike (dense); a linear grid, the
// target prime fastest (moddown_rb2)
// K is the FLOOR kernel (what agx_ntt_basis_mod_down always launched), KR the ROUND one; the matrix is ModDown's own (bv.down_mat: t D_i mod q_j)
template <class S, auto K, auto KR>
hipError_t launch_moddown_t(const plan_view& pv, const basis_view& bv, const uint64_t* xq, const uint64_t* y, uint64_t* out, const frame_layout& fl, bool round,
                            hipStream_t s) {
    const uint64_t blocks = (uint64_t)bv.dst_count * ((fl.batch + S::fpb - 1) / S::fpb);
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (round)
        hipLaunchKernelGGL(KR, dim3((unsigned)blocks), dim3(S::threads), S::lds, s, xq, y, out, pv.consts, bv.down_mat, bv.dall, pv.tw_rb, pv.rb->table_pairs, fl.batch,
                           fl.prime_stride, fl.poly_stride, bv.src_count, bv.dst_first, bv.dst_count, bv.round_src, bv.round_dst);
    else
        hipLaunchKernelGGL(K, dim3((unsigned)blocks), dim3(S::threads), S::lds, s, xq, y, out, pv.consts, bv.down_mat, bv.dall, pv.tw_rb, pv.rb->table_pairs, fl.batch,
                           fl.prime_stride, fl.poly_stride, bv.src_count, bv.dst_first, bv.dst_count);
    return hipGetLastError();
}

template <int L, int R, int ARITH, int MINW>
hipError_t launch_mul_park_t(const plan_view& pv, const uint64_t* a, const uint64_t* b, uint64_t* c, const frame_layout& fl, hipStream_t s) {
    using S = rb2_shape<L, R, 1, ARITH, MINW>;
    if (a == b)      // squaring: NTT(a) times itself in registers (the parked form would read its own parked words back when c aliases too)
        return launch_frames<S>(&polysquare_rb2<L, R, ARITH, MINW>, pv, fl, s, a, c, pv.consts, pv.tw_rb, pv.itw_rb, pv.rb->table_pairs, fl.batch,
                                fl.prime_stride, fl.poly_stride);
    // the operand c aliases (if any) must be the one that is read completely before c's frame is written
    const uint64_t* first = (c == b) ? b : a;
    const uint64_t* second = (c == b) ? a : b;
    return launch_frames<S>(&polymul_rb2_park<L, R, ARITH, MINW>, pv, fl, s, first, second, c, pv.consts, pv.tw_rb, pv.itw_rb, pv.rb->table_pairs,
                            fl.batch, fl.prime_stride, fl.poly_stride);
}

// The loop kernels' launch: a resident grid -- as many workgroups as the current device holds at once at S::min_waves waves per SIMD, at most
// one per frame -- over `total` = batch x primes frames, which the kernels number in 32 bits
template <class S>
hipError_t resident_grid(const plan_view& pv, const frame_layout& fl, unsigned* grid, uint32_t* total) {
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    const uint64_t frames = fl.batch * pv.num_primes, resident = (uint64_t)cus * (unsigned)(S::min_waves * 256 / S::threads);
    if (frames >= (1ull << 31)) return hipErrorInvalidValue;
    *total = (uint32_t)frames;
    *grid = (unsigned)(frames < resident ? frames : resident);
    return hipSuccess;
}

template <int L, int R, int ARITH, int MINW>
hipError_t launch_inv_rb2_loop_t(const plan_view& pv, const uint64_t* in, const uint64_t* in2, uint64_t* out, const frame_layout& fl, hipStream_t s) {
    using S = rb2_shape<L, R, 1, ARITH, MINW>;
    unsigned grid = 0;
    uint32_t total = 0;
    const hipError_t e = resident_grid<S>(pv, fl, &grid, &total);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((inv_rb2_loop<L, R, ARITH, MINW>), dim3(grid), dim3(S::threads), S::lds, s, in, in2, out, pv.consts, pv.itw_rb,
                       pv.rb->table_pairs, (uint32_t)fl.batch, total, fl.prime_stride, fl.poly_stride);
    return hipGetLastError();
}

// A launch recorded into a hipGraph would keep its ticket pair for as long as the graph lives, while eager launches of the same
// stream keep drawing from it; captured launches therefore take the fixed-stride loop kernel, which carries no state.
inline bool stream_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st == hipStreamCaptureStatusActive;
}

constexpr size_t kDloopMailboxBytes = 16;      // inv_rb2_dloop's two-slot mailbox behind the frame's image

template <int L, int R, int ARITH, int MINW>
hipError_t launch_inv_rb2_dloop_t(const plan_view& pv, const uint64_t* in, const uint64_t* in2, uint64_t* out, const frame_layout& fl, hipStream_t s) {
    using S = rb2_shape<L, R, 1, ARITH, MINW>;
    if (stream_is_capturing(s)) return launch_inv_rb2_loop_t<L, R, ARITH, MINW>(pv, in, in2, out, fl, s);
    unsigned grid = 0;
    uint32_t total = 0;
    hipError_t e = resident_grid<S>(pv, fl, &grid, &total);
    if (e != hipSuccess) return e;
    uint32_t* ticket = pv.ticket(s);      // taken last: from here on the launch is issued and ticket_done() follows it
    if (!ticket) return launch_inv_rb2_loop_t<L, R, ARITH, MINW>(pv, in, in2, out, fl, s);      // no pair provably free: stateless form
    hipLaunchKernelGGL((inv_rb2_dloop<L, R, ARITH, MINW>), dim3(grid), dim3(S::threads), S::lds + kDloopMailboxBytes, s, in, in2, out, pv.consts, pv.itw_rb,
                       pv.rb->table_pairs, (uint32_t)fl.batch, total, fl.prime_stride, fl.poly_stride, ticket);
    e = hipGetLastError();
    pv.ticket_done(s, ticket);      // an event behind the launch: when it has fired the pair is idle (and zero) and the plan may hand it to another stream
    return e;
}

// ---- registry entries: each is built from exactly the kernels it launches, so nothing else is instantiated ----------------------------
template <class S>
constexpr rb_entry shape_entry(int id, decltype(rb_entry::launch) fwd, decltype(rb_entry::init) init, decltype(rb_entry::launch_inv) inv,
                               decltype(rb_entry::launch_mul) mul, decltype(rb_entry::launch_mulhat) mulhat = nullptr,
                               decltype(rb_entry::launch_rescale) rescale = nullptr, decltype(rb_entry::launch_extend) extend = nullptr,
                               decltype(rb_entry::launch_moddown) moddown = nullptr) {
    return rb_entry{id, S::log_n, S::r, S::fpb, S::min_waves, S::table_pairs, S::lds, S::build, fwd, init, S::arith, inv, mul, 0, 0, S::narrow, mulhat, rescale, extend, moddown};
}

// forward, inverse and the product with both forward results in registers, one workgroup per S::fpb frames each (every family has this form)
template <class S, auto FWD, auto INV, auto MUL>
constexpr rb_entry make_entry3(int id) {
    return shape_entry<S>(id, &launch_fwd_t<S, FWD>, &allow_lds<S::lds, FWD, INV, MUL>, &launch_inv_t<S, INV>, &launch_mul_t<S, MUL>);
}

// PPB frames per workgroup (the n = 4096 defaults: R = 3, 8 waves/SIMD; n = 1024 with streamed twiddles, where two frames of 2^R coefficients still fit
// the register budget and the parked product's round trip through c's frame would cost more); the product kernel at MULW waves per SIMD
// and the product by a pre-transformed operand, the rescale kernel and the base-extension and ModDown kernels (one frame in registers; at most AGX_MULHAT_MAXW waves per SIMD)
template <int L, int R, int PPB, int ARITH, int MINW, int MULW = MINW>
constexpr rb_entry make_entry2(int id) {
    using S = rb2_shape<L, R, PPB, ARITH, MINW>;
    constexpr auto fwd = &fwd_rb2<L, R, PPB, ARITH, MINW>;
    constexpr auto inv = &inv_rb2<L, R, PPB, ARITH, MINW>;
    constexpr auto mul = &polymul_rb2<L, R, PPB, ARITH, MULW>;
    constexpr auto mulhat = &mulhat_rb2<L, R, PPB, ARITH, MINW>;
    constexpr auto rescale = &rescale_rb2<L, R, PPB, ARITH, MINW>;
    constexpr auto extend = &extend_rb2<L, R, PPB, ARITH, MINW>;
    constexpr auto moddown = &moddown_rb2<L, R, PPB, ARITH, MINW>;
    constexpr auto moddown_round = &moddown_round_rb2<L, R, PPB, ARITH, MINW>;
    return shape_entry<S>(id, &launch_fwd_t<S, fwd>, &allow_lds<S::lds, fwd, inv, mul, mulhat, rescale, extend, moddown, moddown_round>, &launch_inv_t<S, inv>, &launch_mul_t<S, mul>, &launch_mulhat_t<S, mulhat>,
                          &launch_rescale_t<S, rescale>, &launch_extend_t<S, extend>, &launch_moddown_t<S, moddown, moddown_round>);
}

// forward kernel only (a plan's forward companion: rb_entry::fwd_companion), one frame per workgroup
template <int L, int R, int ARITH, int MINW>
constexpr rb_entry make_entry_single_fwd(int id) {
    using S = rb2_shape<L, R, 1, ARITH, MINW>;
    constexpr auto fwd = &fwd_rb2<L, R, 1, ARITH, MINW>;
    return shape_entry<S>(id, &launch_fwd_t<S, fwd>, &allow_lds<S::lds, fwd>, nullptr, nullptr);
}

// ... with two kernels of one shape and one table behind the id, chosen on the host per launch: the skip form of the two-twiddle butterfly
// (ARITH | kOptQ60cSkip) for plans whose moduli are all 2^60 - c with c <= kQ60cSkipMaxC (plan_view::q60c_skip), the kernel of ARITH itself for every other
// plan the entry may serve -- mixed plans included, bit for bit what the entry launched before it had the first.  No kernel branches on c.
template <class S, auto SKIP, auto GENERAL>
hipError_t launch_fwd_q60c_skip_t(const plan_view& pv, const uint64_t* in, uint64_t* out, const frame_layout& fl, hipStream_t s) {
    return pv.q60c_skip ? launch_fwd_t<S, SKIP>(pv, in, out, fl, s) : launch_fwd_t<S, GENERAL>(pv, in, out, fl, s);
}
template <int L, int R, int ARITH, int MINW>
constexpr rb_entry make_entry_single_fwd_q60c_skip(int id) {
    constexpr int ARITH_SKIP = ARITH | (kOptQ60cSkip << 1);
    using S = rb2_shape<L, R, 1, ARITH, MINW>;
    using SS = rb2_shape<L, R, 1, ARITH_SKIP, MINW>;
    static_assert(frame_of<L, R, ARITH>::Q60C_FOLD && !frame_of<L, R, ARITH>::Q60C_SKIP && frame_of<L, R, ARITH_SKIP>::Q60C_SKIP, "the general kernel is the two-twiddle form without the skip");
    static_assert(S::lds == SS::lds && S::threads == SS::threads && S::table_pairs == SS::table_pairs && S::build == SS::build && S::arith == SS::arith,
                  "one launch shape and one pass table serve both kernels");
    constexpr auto skip = &fwd_rb2<L, R, 1, ARITH_SKIP, MINW>;
    constexpr auto general = &fwd_rb2<L, R, 1, ARITH, MINW>;
    return shape_entry<S>(id, &launch_fwd_q60c_skip_t<S, skip, general>, &allow_lds<S::lds, skip, general>, nullptr, nullptr);
}

// the streamed single-frame kernels (reg_s<n>.hip): one frame in registers per workgroup at any time (R = 5: a second frame cannot
// be held): forward, inverse, the fused product by polymul_rb2_park / polysquare_rb2, the product by a pre-transformed operand, the rescale kernel, the base-extension and ModDown kernels
template <int L, int R, int ARITH, int MINW>
constexpr rb_entry make_entry_single(int id) {
    using S = rb2_shape<L, R, 1, ARITH, MINW>;
    constexpr auto fwd = &fwd_rb2<L, R, 1, ARITH, MINW>;
    constexpr auto inv = &inv_rb2<L, R, 1, ARITH, MINW>;
    constexpr auto mulhat = &mulhat_rb2<L, R, 1, ARITH, MINW>;
    constexpr auto rescale = &rescale_rb2<L, R, 1, ARITH, MINW>;
    constexpr auto extend = &extend_rb2<L, R, 1, ARITH, MINW>;
    constexpr auto moddown = &moddown_rb2<L, R, 1, ARITH, MINW>;
    constexpr auto moddown_round = &moddown_round_rb2<L, R, 1, ARITH, MINW>;
    return shape_entry<S>(id, &launch_fwd_t<S, fwd>, &allow_lds<S::lds, fwd, inv, &polymul_rb2_park<L, R, ARITH, MINW>, &polysquare_rb2<L, R, ARITH, MINW>, mulhat, rescale, extend, moddown, moddown_round>,
                          &launch_inv_t<S, inv>, &launch_mul_park_t<L, R, ARITH, MINW>, &launch_mulhat_t<S, mulhat>, &launch_rescale_t<S, rescale>, &launch_extend_t<S, extend>,
                          &launch_moddown_t<S, moddown, moddown_round>);
}

// entry e with forward calls of its plans routed to the forward-only entry `id` (rb_entry::fwd_companion)
constexpr rb_entry with_fwd_companion(rb_entry e, int id, uint32_t min_frames = 0) {
    e.fwd_companion = id;
    e.fwd_companion_min_frames = min_frames;
    return e;
}

// ... with the inverse by the ticket-drawing loop kernel (captured launches and streams without a ticket pair take the fixed-stride form)
template <int L, int R, int ARITH, int MINW>
hipError_t init_rb2_single_invloop_t() {
    using S = rb2_shape<L, R, 1, ARITH, MINW>;
    const hipError_t e = allow_lds<S::lds, &fwd_rb2<L, R, 1, ARITH, MINW>, &inv_rb2_loop<L, R, ARITH, MINW>, &polymul_rb2_park<L, R, ARITH, MINW>,
                                   &polysquare_rb2<L, R, ARITH, MINW>, &mulhat_rb2<L, R, 1, ARITH, MINW>, &rescale_rb2<L, R, 1, ARITH, MINW>, &extend_rb2<L, R, 1, ARITH, MINW>,
                                   &moddown_rb2<L, R, 1, ARITH, MINW>, &moddown_round_rb2<L, R, 1, ARITH, MINW>>();
    return e != hipSuccess ? e : allow_lds<S::lds + kDloopMailboxBytes, &inv_rb2_dloop<L, R, ARITH, MINW>>();
}
template <int L, int R, int ARITH, int MINW>
constexpr rb_entry make_entry_single_invloop(int id) {
    using S = rb2_shape<L, R, 1, ARITH, MINW>;
    return shape_entry<S>(id, &launch_fwd_t<S, &fwd_rb2<L, R, 1, ARITH, MINW>>, &init_rb2_single_invloop_t<L, R, ARITH, MINW>,
                          &launch_inv_rb2_dloop_t<L, R, ARITH, MINW>, &launch_mul_park_t<L, R, ARITH, MINW>, &launch_mulhat_t<S, &mulhat_rb2<L, R, 1, ARITH, MINW>>,
                          &launch_rescale_t<S, &rescale_rb2<L, R, 1, ARITH, MINW>>, &launch_extend_t<S, &extend_rb2<L, R, 1, ARITH, MINW>>,
                          &launch_moddown_t<S, &moddown_rb2<L, R, 1, ARITH, MINW>, &moddown_round_rb2<L, R, 1, ARITH, MINW>>);
}

}  // namespace AGX_TU
}  // namespace agx
