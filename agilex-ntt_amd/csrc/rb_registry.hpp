// rb_registry.hpp -- the registry of register-blocked kernel configurations, shared by the translation
// units that instantiate the kernels (reg_*.hip) and the one that looks entries up (ntt_kernels.hip).
#pragma once
#include "ntt_kernels.hpp"

namespace agx {

// ---- registry of register-blocked configurations -------------------------------------
// ids are stable handles (agx_ntt_plan_set_variant(plan, AGX_VARIANT_REGBLOCK_BASE + id); rocprof summaries and tests name them),
// not indices.  Every entry transforms WHOLE frames of n = 2^log_n coefficients resident on chip.
struct rb_entry {
    int id, log_n, r, ppb;   // ppb: frames per workgroup
    int min_waves;
    uint32_t table_pairs;   // pass-table length per prime, in {w,w'} pairs
    size_t lds_bytes;
    void (*build)(const uint64_t* tw, const uint64_t* pre, uint64_t q, std::vector<ulonglong2>& out);      // appends the pass table of one prime q
    hipError_t (*launch)(const plan_view&, const uint64_t*, uint64_t*, const frame_layout&, hipStream_t);
    hipError_t (*init)();    // allows every kernel the entry launches the dynamic LDS it is launched with
    int arith;   // 0: exact (reference op sequence, q < 2^62); 1: fast (q <= 2^61); 2: 16q-lazy (q <= 2^60); 3: 16q-lazy for q = 2^60 - c, 0 < c < 2^28
    hipError_t (*launch_inv)(const plan_view&, const uint64_t*, const uint64_t*, uint64_t*, const frame_layout&, hipStream_t);      // in2 != null: in * in2 is transformed
    hipError_t (*launch_mul)(const plan_view&, const uint64_t*, const uint64_t*, uint64_t*, const frame_layout&, hipStream_t);      // c = INTT(NTT(a) o NTT(b)) in one launch
    int fwd_companion = 0;     // registry id of a forward-only entry that serves forward calls of a plan whose main entry is this one (0: none)
    uint32_t fwd_companion_min_frames = 0;   // ... for launches of at least this many frames (batch x primes): a shape with fewer threads per frame wins
                                             // on throughput but loses on the latency of a launch that does not fill the chip
    int narrow = 0;            // 0: 64-bit arithmetic; 1: 32-bit arithmetic, every modulus < 2^31; 2: every modulus < 2^30 (rb32_kernels.hpp)
    // c = INTT(NTT(a) o bhat) in one launch, bhat already transformed (frame (p, f) of bhat at p * bhat_prime_stride + f * bhat_poly_stride,
    // a poly stride of 0 = one bhat frame per prime for the whole batch); null: the entry's plans take the generic three-launch path
    hipError_t (*launch_mulhat)(const plan_view&, const uint64_t*, const uint64_t*, uint64_t*, const frame_layout&, int64_t bhat_prime_stride,
                                int64_t bhat_poly_stride, hipStream_t) = nullptr;
    // agx_ntt_rescale's second launch on a view of primes 0 .. P-2: out_i = (x_i - NTT_i(lift of t to q_i)) q_L^-1, t ([batch][n], poly stride as
    // the frame layout's) the coefficients of the last slab; out may be x.  null: the entry's plans take the generic route
    hipError_t (*launch_rescale)(const plan_view&, const uint64_t* x, const uint64_t* t, uint64_t* out, const frame_layout&, bool round, hipStream_t) = nullptr;
    // agx_ntt_basis_extend to NTT form in one launch, on a view of the WHOLE plan: out_j = NTT_j(sum_i y_i (D_i mod q_j)) for the basis' targets, x
    // dense [S][batch][n] in coefficient form, out dense [T][batch][n] (the frame layout's strides serve both), out of place.  The caller keeps
    // T ceil(batch / ppb) workgroups within the grid limit.  null: the entry's plans run launch_basis_coeff, then the forward in place
    hipError_t (*launch_extend)(const plan_view&, const basis_view&, const uint64_t* x, uint64_t* out, const frame_layout&, hipStream_t) = nullptr;
    // agx_ntt_basis_mod_down's second launch, on a view of the WHOLE plan: out_j = (xq_j - NTT_j(sum_i y_i (D_i mod q_j))) D^-1 mod q_j for the basis'
    // targets, y dense [S][batch][n] (the scaled coefficient form of the source slabs, y_i in [0,q_i)), xq and out dense [T][batch][n] in NTT form (the
    // frame layout's strides serve all three); out may be xq.  The caller keeps T ceil(batch / ppb) workgroups within the grid limit.  null: the
    // entry's plans take the generic route.  The matrix is the basis' down_mat (t D_i mod q_j); round: AGX_RESCALE_ROUND, a kernel of its own that also
    // reads round_src and round_dst (moddown_round_rb2) -- without it the kernel agx_ntt_basis_mod_down always launched
    hipError_t (*launch_moddown)(const plan_view&, const basis_view&, const uint64_t* xq, const uint64_t* y, uint64_t* out, const frame_layout&, bool round,
                                 hipStream_t) = nullptr;
};

// The view of primes [lo, hi) of a route: every per-prime array starts at prime lo, so the launchers run on one slab or on the first
// slabs of a call unchanged (the ticket plumbing stays the plan's).
inline plan_view prime_range(plan_view v, uint32_t lo, uint32_t hi) {
    v.consts += lo;
    v.tw += (size_t)lo * v.n;
    if (v.itw) v.itw += (size_t)lo * v.n;
    if (v.tw_rb) v.tw_rb += (size_t)lo * v.rb->table_pairs;
    if (v.itw_rb) v.itw_rb += (size_t)lo * v.rb->table_pairs;
    if (v.rescale) v.rescale += lo;
    v.num_primes = hi - lo;
    return v;
}

struct rb_span {
    const rb_entry* first;
    size_t count;
};

// one group per translation unit, so the ~50 kernel instantiations compile in parallel
// product groups (their A/B extras are compiled in under AGX_DIAG)
rb_span rb_entries_n4096();
rb_span rb_entries_s1024();      // the streamed single-frame kernels, one group (translation unit) per size
rb_span rb_entries_s2048();
rb_span rb_entries_s4096();
rb_span rb_entries_s8192();
rb_span rb_entries_s16384();
rb_span rb_entries_s32768();
rb_span rb_entries_q32a();       // 32-bit arithmetic, tier 2 (every modulus < 2^30) / tier 1 (< 2^31)
rb_span rb_entries_q32b();
rb_span rb_entries_wp();         // wave-packed kernels of n = 32 ... 512 (wp_kernels.hpp): 64-bit arithmetic / 32-bit arithmetic
rb_span rb_entries_wp32();
#ifdef AGX_DIAG
rb_span rb_entries_diag();                                      // lib/libagxntt_diag.so only: the trace twin of the n = 4096 default (tools/timeline.py)
hipError_t regblock_set_trace(uint64_t* buf, uint64_t waves);   // where the trace kernel writes
#endif

}  // namespace agx
