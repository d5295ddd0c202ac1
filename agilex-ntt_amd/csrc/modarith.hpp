// modarith.hpp -- 64-bit lazy modular arithmetic for gfx950 (device side).
//
// Value ranges follow the reference butterfly (src/kernel/ntt.cpp:302-369): coefficients live
// in [0,4q) between stages, q < 2^62 so nothing overflows 64 bits, and only the last stage
// reduces to [0,q) (src/kernel/ntt.cpp:377-394).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "q60c_class.hpp"      // kQ60cSkipMaxC: the class limit that q60c_skip_bounds proves and the host tests

namespace agx {

// {w, w'} with w' = floor(w * 2^64 / q): one 16-byte load fetches both
typedef ulonglong2 twpair;

// w*y - floor(w'*y / 2^64) * q  (mod 2^64)  in [0,2q) for any 64-bit y   (ntt.cpp:344-363)
__device__ __forceinline__ uint64_t mul_shoup_lazy(uint64_t y, uint64_t w, uint64_t wp, uint64_t q) {
    const uint64_t c = __umul64hi(y, wp);
    return w * y - c * q;
}

__device__ __forceinline__ uint64_t csub(uint64_t v, uint64_t m) { return v >= m ? v - m : v; }

// [0,4q) -> [0,q)   (ntt.cpp:377-394)
__device__ __forceinline__ uint64_t reduce_4q(uint64_t v, uint64_t q, uint64_t q2) {
    return csub(csub(v, q2), q);
}

// Cooley-Tukey (decimation in time) Harvey butterfly: x,y in [0,4q) -> [0,4q)
__device__ __forceinline__ void ct_butterfly(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp,
                                             uint64_t q, uint64_t q2) {
    const uint64_t tx = csub(x, q2);                  // ntt.cpp:331-332
    const uint64_t qv = mul_shoup_lazy(y, w, wp, q);  // ntt.cpp:344-363
    x = tx + qv;                                      // ntt.cpp:368
    y = tx + q2 - qv;                                 // ntt.cpp:369
}

// Gentleman-Sande (decimation in frequency) butterfly for the inverse: x,y in [0,2q) -> [0,2q)
__device__ __forceinline__ void gs_butterfly(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp,
                                             uint64_t q, uint64_t q2) {
    const uint64_t s = csub(x + y, q2);
    const uint64_t d = x + q2 - y;  // (0,4q)
    x = s;
    y = mul_shoup_lazy(d, w, wp, q);
}

// per-prime constants for a*b mod q with both operands variable
struct barrett128 {
    uint64_t q;
    uint64_t mu_hi, mu_lo;  // floor(2^128 / q)
};

// a*b mod q in [0,q) for a, b < q < 2^62, and also for a, b < 4q when q <= 2^60 (then a*b < 2^124 and
// the quotient < 16q <= 2^64 still fit).  Quotient estimate is low by at most 3.
__device__ __forceinline__ uint64_t mul_mod_barrett(uint64_t a, uint64_t b, const barrett128& k) {
    const uint64_t lo = a * b, hi = __umul64hi(a, b);
    const uint64_t est = hi * k.mu_hi + __umul64hi(hi, k.mu_lo) + __umul64hi(lo, k.mu_hi);
    uint64_t r = lo - est * k.q;  // [0,4q)
    r = csub(r, k.q << 1);
    return csub(r, k.q);
}


// v mod q in [0,q) for ANY 64-bit v and any q < 2^62 (whatever the ratio v / q): mu_hi = floor(2^64 / q), so the estimate
// e = floor(v mu_hi / 2^64) lies in (v/q - v/2^64 - 1, v/q]: e is floor(v/q) or one less, v - e q in [0,2q) < 2^63.
__device__ __forceinline__ uint64_t reduce_u64(uint64_t v, const barrett128& k) {
    return csub(v - __umul64hi(v, k.mu_hi) * k.q, k.q);
}

// Exact division by the last RNS modulus q_L (agx_ntt_rescale), per coefficient.
// lift: t in [0,q_L) (a coefficient of the last slab) -> u = ((t + h) mod q_L) mod q - (h mod q)  mod q, in [0,q); floor mode passes
// h = hq = 0.  t + h < 2 q_L < 2^63; one conditional subtract brings it under q_L, reduce_u64 under q for any ratio q_L / q.
__device__ __forceinline__ uint64_t rescale_lift(uint64_t t, uint64_t h, uint64_t hq, uint64_t q_last, const barrett128& k) {
    const uint64_t a = reduce_u64(csub(t + h, q_last), k);      // [0,q)
    return a - hq + (a < hq ? k.q : 0);                           // hq < q: [0,q)
}
// finish: (x - z) q_L^-1 mod q in [0,q), {w, wp} = q_L^-1 mod q and its quotient.  LAZY (q <= 2^60 only): x, z in [0,4q), d = x + 4q - z
// in (0,8q) <= 2^63.  Otherwise x, z in [0,q) and d = x + q - z in (0,2q) < 2^63: 4q is never formed, so q may be anything below 2^62.
// mul_shoup_lazy takes any 64-bit d to [0,2q).
template <bool LAZY>
__device__ __forceinline__ uint64_t rescale_finish(uint64_t x, uint64_t z, uint64_t w, uint64_t wp, uint64_t q) {
    const uint64_t d = x + (LAZY ? q << 2 : q) - z;
    return csub(mul_shoup_lazy(d, w, wp, q), q);
}

// Fast RNS base conversion (agx_ntt_basis_extend), per coefficient: out_j = sum_i y_i (D_i mod q_j) mod q_j with y_i = x_i D_i^-1 mod q_i.
// scale: a source word x (any 64-bit value: [0,4q_i) as the transforms accept it) -> y_i in [0,q_i), fully reduced -- the sum is an integer
// formula in the y_i, so their representative matters.  {w, wp} = D_i^-1 mod q_i and its quotient.
__device__ __forceinline__ uint64_t basis_scale(uint64_t x, uint64_t w, uint64_t wp, uint64_t qi) {
    return csub(mul_shoup_lazy(x, w, wp, qi), qi);
}
// accumulate: acc in [0,2q) -> acc + y (D_i mod q_j) mod q_j in [0,2q).  y is a residue of ANOTHER modulus (any value below 2^62), which
// mul_shoup_lazy takes to [0,2q); the sum stays below 4q < 2^64.  {c, cp} = D_i mod q_j and its quotient.  One conditional subtract per
// term instead of a 128-bit sum and one reduction per word: half the accumulator registers, which the fused kernel needs (rb_kernels.hpp).
__device__ __forceinline__ uint64_t basis_accumulate(uint64_t acc, uint64_t y, uint64_t c, uint64_t cp, uint64_t q, uint64_t q2) {
    return csub(acc + mul_shoup_lazy(y, c, cp, q), q2);
}

// ---------------------------------------------------------------------------------------
// Hand-selected instruction forms for the throughput kernels.
//
// Box calibration (profiles/r01_microbench_box_calibration.txt): on gfx950 every VOP3 integer
// op (v_mad_u64_u32, v_mul_lo/hi_u32, v_add3, v_lshl_add_u64, carry adds) issues at about half
// the rate of a plain VOP2 add, so a butterfly's cost is its instruction COUNT.  hipcc lowers
// the portable butterfly above to ~32 VALU instructions (v_mul_lo + v_add3 cross terms,
// v_mov pairs to zero-extend 32-bit partial products, 64-bit compare + 2 selects); the forms
// below need about 20 (fast) / 27 (exact).  They stay in C++ (two opaque values steer hipcc's
// instruction selection) because hipcc pads every inline-asm instruction with an s_nop.
// ---------------------------------------------------------------------------------------

// a*b + c with a,b 32-bit: hipcc selects v_mad_u64_u32 for this shape
__device__ __forceinline__ uint64_t mad64(uint32_t a, uint32_t b, uint64_t c) { return (uint64_t)a * b + c; }
__device__ __forceinline__ uint64_t mul64(uint32_t a, uint32_t b) { return (uint64_t)a * b; }

// The value 1 in a form the optimiser cannot see through: c + zext(a) is then one
// v_mad_u64_u32 (a * 1 + c) instead of a v_mov (to build the {a,0} pair) plus a 64-bit add.
template <int TAG>   // identical asm statements would be merged: give each value its own text
__device__ __forceinline__ uint32_t opaque_one() {
    uint32_t one;
    if constexpr (TAG == 0) asm("s_mov_b32 %0, 1" : "=s"(one));
    else asm("s_movk_i32 %0, 0x1" : "=s"(one));
    return one;
}
// Two such adds in one sum must use DIFFERENT opaque ones, or hipcc factors them back into
// (a + b) * one and rebuilds the register pairs this is meant to avoid.
__device__ __forceinline__ uint64_t add64_32(uint64_t c, uint32_t a, uint32_t one) { return (uint64_t)a * one + c; }

// hide how a wave-uniform 64-bit constant was derived (x + opaque(-m) stays ONE v_lshl_add_u64
// instead of becoming a v_sub_co/v_subb pair)
__device__ __forceinline__ uint64_t opaque_sgpr64(uint64_t v) {
    asm("" : "+s"(v));
    return v;
}

// Keeps all 64 bits of v live, so a multiply-add chain of which only the low word is used is
// not demoted to v_mul_lo_u32 + v_add3_u32 pairs (two instructions per term instead of one).
__device__ __forceinline__ uint64_t keep64(uint64_t v) {
    asm("" : "+v"(v));
    return v;
}

// per-prime constants of the throughput kernels (wave-uniform: live in SGPRs)
struct bf_consts {
    uint64_t q;
    uint64_t nq;     // 2^64 - q
    uint64_t m;      // lazy-range step: 2q (exact arithmetic) or 4q (fast arithmetic)
    uint64_t nm;     // 2^64 - m
    uint32_t one_a, one_b;  // two separate opaque_one() values (see add64_32)
    float est_inv;          // slightly below 2^32 / q, or 0 when q < 2^58 (reduce_final_est)
    uint32_t c, c8;         // q = 2^60 - c kernels only (below): c and 8c
    uint32_t c2, p29;       // two-twiddle form of those kernels only (ct_butterfly_q60c_fold): 2c, and 2^29 in a form the optimiser cannot see through
    uint64_t mfold;         // ... and its lazy-range constant: 8q (sign-bit subtract on every stage), or 7q (top-four-bit reduction on every second stage)
};

// x in [0,2m) -> x - (x >= m ? m : 0) through the sign of x - m; needs 2m <= 2^63... see callers
__device__ __forceinline__ uint64_t csub_sign(uint64_t x, const bf_consts& k) {
    const uint64_t d = x + k.nm;
    const uint32_t neg = (uint32_t)((int32_t)(uint32_t)(d >> 32) >> 31);  // all ones when x < m
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 add;
    add.x = neg & (uint32_t)k.m;
    add.y = neg & (uint32_t)(k.m >> 32);
    return d + __builtin_bit_cast(uint64_t, add);
}

// x' = tx + w*y - c*q (mod 2^64), the whole right-hand side in 6 multiply-adds + 1 add:
// the low words accumulate straight onto tx, the four cross products only matter mod 2^32
// VAR (A/B in tools/microbench pwr, energy per butterfly): 0 = the four cross products as one v_mad_u64_u32 chain (shipped);
// 1 = as 32-bit products (v_mul_lo_u32 + adds: more instructions, narrower results)
template <int VAR = 0>
__device__ __forceinline__ uint64_t fold_product(uint64_t tx, uint64_t y, uint64_t w, uint64_t c, const bf_consts& k) {
    const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32), w0 = (uint32_t)w, w1 = (uint32_t)(w >> 32);
    const uint32_t c0 = (uint32_t)c, c1 = (uint32_t)(c >> 32), nq0 = (uint32_t)k.nq, nq1 = (uint32_t)(k.nq >> 32);
    uint64_t acc = mad64(w0, y0, tx);
    acc = mad64(nq0, c0, acc);
    if constexpr (VAR == 1) {
        const uint32_t z32 = w0 * y1 + w1 * y0 + nq1 * c0 + nq0 * c1;
        typedef uint32_t u32x2v __attribute__((ext_vector_type(2)));
        u32x2v av = __builtin_bit_cast(u32x2v, acc);
        av.y += z32;
        return __builtin_bit_cast(uint64_t, av);
    }
    uint64_t z = mul64(w0, y1);
    z = mad64(w1, y0, z);
    z = mad64(nq1, c0, z);
    z = keep64(mad64(nq0, c1, z));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 a = __builtin_bit_cast(u32x2, acc);
    a.y += (uint32_t)z;
    return __builtin_bit_cast(uint64_t, a);
}

// EXACT arithmetic: the reference's butterfly (src/kernel/ntt.cpp:331-369) value for value --
// c = floor(y*w'/2^64) exactly, coefficients in [0,4q), any q < 2^62.
__device__ __forceinline__ void ct_butterfly_exact(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp, const bf_consts& k) {
    const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32), p0 = (uint32_t)wp, p1 = (uint32_t)(wp >> 32);
    const uint64_t tx = csub(x, k.m);                                       // m = 2q
    const uint32_t t = __umulhi(y0, p0);
    const uint64_t m1 = add64_32(mul64(p1, y0), t, k.one_a);                 // y0*p1 + hi(y0*p0)
    const uint64_t m2 = add64_32(mul64(p0, y1), (uint32_t)m1, k.one_b);      // y1*p0 + lo(m1)
    uint64_t c = add64_32(mul64(p1, y1), (uint32_t)(m1 >> 32), k.one_a);
    c = add64_32(c, (uint32_t)(m2 >> 32), k.one_b);
    const uint64_t xn = fold_product(tx, y, w, c, k);
    y = (tx << 1) + k.m - xn;                                               // tx + 2q - Q
    x = xn;
}

// FAST arithmetic for q <= 2^61: quotient estimate c~ = y1*p1 + hi(y0*p1) + hi(y1*p0) is low by
// at most 2, so Q~ = w*y - c~*q lies in [0,4q); coefficients are kept in [0,8q) with m = 4q:
//   tx = x - (x >= 4q ? 4q : 0) < 4q,  x' = tx + Q~ < 8q,  y' = tx + 4q - Q~ in (0,8q).
// Same residues as the exact form at every stage, so the fully reduced outputs are identical.
// x in [0,2m) -> x - (x >= m ? m : 0) by selecting on the sign of x - m (compare + two selects)
__device__ __forceinline__ uint64_t csub_select(uint64_t x, const bf_consts& k) {
    const uint64_t d = x + k.nm;
    return (int64_t)d < 0 ? x : d;
}

template <bool SEL = false>
__device__ __forceinline__ void ct_butterfly_fast(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp, const bf_consts& k) {
    const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32), p0 = (uint32_t)wp, p1 = (uint32_t)(wp >> 32);
    const uint64_t tx = SEL ? csub_select(x, k) : csub_sign(x, k);          // m = 4q <= 2^63
    uint64_t c = mad64(p1, y1, (uint64_t)__umulhi(y0, p1));                  // one v_mov builds the {h,0} pair
    c = add64_32(c, __umulhi(y1, p0), k.one_b);
    const uint64_t xn = fold_product(tx, y, w, c, k);
    y = (tx << 1) + k.m - xn;                                               // tx + 4q - Q~
    x = xn;
}

// [0,2m) -> [0,q) at the last stage (m = 2q: two steps; m = 4q: three).  The fast form may use
// the sign trick for every step (all values < 2^63 after the first one); the exact form must
// compare (q may exceed 2^61).
__device__ __forceinline__ uint64_t csub_sign_c(uint64_t x, uint64_t m, uint64_t nm) {
    const uint64_t d = x + nm;
    const uint32_t neg = (uint32_t)((int32_t)(uint32_t)(d >> 32) >> 31);
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 add;
    add.x = neg & (uint32_t)m;
    add.y = neg & (uint32_t)(m >> 32);
    return d + __builtin_bit_cast(uint64_t, add);
}

struct final_consts {   // fast forms only
    uint64_t q2, nq2, q1, nq1;
    uint64_t q8, nq8;   // 8q and its negation: the conditional-subtract step of the 16q-lazy form
};

template <bool FAST, bool SEL = false>
__device__ __forceinline__ uint64_t reduce_final(uint64_t v, const bf_consts& k, const final_consts& f, bool lazy_out = false) {
    if constexpr (FAST && SEL) {
        const uint64_t d4 = v + k.nm;            // [0,8q) -> [0,4q)
        v = (int64_t)d4 < 0 ? v : d4;
        if (lazy_out) return v;
        const uint64_t d2 = v + f.nq2;
        v = (int64_t)d2 < 0 ? v : d2;
        const uint64_t d1 = v + f.nq1;
        return (int64_t)d1 < 0 ? v : d1;
    } else if constexpr (FAST) {
        v = csub_sign(v, k);                 // [0,8q) -> [0,4q)
        if (lazy_out) return v;
        v = csub_sign_c(v, f.q2, f.nq2);     // -> [0,2q)
        return csub_sign_c(v, f.q1, f.nq1);  // -> [0,q)
    } else {
        if (lazy_out) return v;              // already in [0,4q)
        v = csub(v, k.q << 1);
        return csub(v, k.q);
    }
}

// 16q-LAZY arithmetic for q <= 2^60 (16q <= 2^64): with twice the headroom of the fast form the
// conditional subtract is only needed when the running bound would pass 16q, which is on 5 of 12
// stages at n = 4096 (lazy16_schedule below) instead of on every stage.  A skipped stage maps a
// bound B to B + 4q (x' = x + Q~, y' = x + 4q - Q~, Q~ < 4q); a subtracting stage uses the step 8q:
// tx = x - [x >= 8q] 8q < max(8q, B - 8q).  Same residues as the other forms at every stage.
struct lazy16_schedule {
    // bound (in units of q) on the coefficients entering stage s, and whether stage s subtracts;
    // inputs are < 4q (the reference's input range, src/kernel/ntt.cpp:331-332)
    static constexpr int bound_in(int s) {
        int b = 4;
        for (int i = 0; i < s; ++i) b = next(b);
        return b;
    }
    static constexpr bool subtracts(int s) { return bound_in(s) + 4 > 16; }
    static constexpr int next(int b) { return (b + 4 > 16 ? (b - 8 > 8 ? b - 8 : 8) : b) + 4; }
};

// TAIL-FREE variant of the schedule for a transform of `total` stages: the same number of subtracting stages, but
// placed on the stages whose parity matches `total` (from stage 2 on), so that the LAST stage never subtracts and its
// outputs are simply below 16q; reduce_final_est then brings them home with one quotient estimate instead of
// 2 + 2x3 conditional subtracts per butterfly.
struct lazy16_tailfree {
    static constexpr bool subtracts(int s, int total) { return s >= 2 && (((s ^ total) & 1) == 0); }
    static constexpr int bound_in(int s, int total) {
        int b = 4;
        for (int i = 0; i < s; ++i) {
            if (subtracts(i, total)) b = b - 8 > 8 ? b - 8 : 8;
            b += 4;
        }
        return b;
    }
    // every stage's outputs stay within 16q, and the last stage does not subtract
    static constexpr bool valid(int total) {
        for (int s = 0; s < total; ++s) {
            const int in = bound_in(s, total);
            if (in > 16) return false;
            if (!subtracts(s, total) && in + 4 > 16) return false;
        }
        return total >= 3 && !subtracts(total - 1, total);
    }
};

// select-based conditional subtract with explicit constants
__device__ __forceinline__ uint64_t csub_select_c(uint64_t x, uint64_t nm) {
    const uint64_t d = x + nm;
    return (int64_t)d < 0 ? x : d;
}

// LAST: the transform's final stage.  There tx is brought below 4q (one more subtract), so the
// outputs are < 8q and the final reduction needs three steps per coefficient instead of four.
template <bool SEL, bool DO_CSUB, bool LAST = false, int VAR = 0>
__device__ __forceinline__ void ct_butterfly_lazy16(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp, const bf_consts& k,
                                                    const final_consts& f) {
    const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32), p0 = (uint32_t)wp, p1 = (uint32_t)(wp >> 32);
    uint64_t tx = x;
    if constexpr (DO_CSUB || LAST) {
        if constexpr (SEL) tx = csub_select_c(tx, f.nq8);
        else tx = csub_sign_c(tx, f.q8, f.nq8);
    }
    if constexpr (LAST) {
        if constexpr (SEL) tx = csub_select_c(tx, k.nm);
        else tx = csub_sign(tx, k);
    }
    uint64_t c = mad64(p1, y1, (uint64_t)__umulhi(y0, p1));                  // one v_mov builds the {h,0} pair
    c = add64_32(c, __umulhi(y1, p0), k.one_b);
    const uint64_t xn = fold_product<VAR>(tx, y, w, c, k);
    y = (tx << 1) + k.m - xn;                                               // tx + 4q - Q~
    x = xn;
}

// after a LAST butterfly: [0,8q) -> [0,q), or only to [0,4q) when the caller asked for lazy outputs
template <bool SEL>
__device__ __forceinline__ uint64_t reduce_final_lazy16(uint64_t v, const bf_consts& k, const final_consts& f, bool lazy_out) {
    if constexpr (SEL) {
        v = csub_select_c(v, k.nm);          // 4q
        if (lazy_out) return v;
        v = csub_select_c(v, f.nq2);
        return csub_select_c(v, f.nq1);
    } else {
        v = csub_sign(v, k);
        if (lazy_out) return v;
        v = csub_sign_c(v, f.q2, f.nq2);
        return csub_sign_c(v, f.q1, f.nq1);
    }
}

// [0,16q) -> [0,q) (or only [0,2q) for lazy outputs) after a tail-free 16q-lazy transform.  For q >= 2^58 the quotient
// floor(v/q) <= 15 is estimated from the top word in single precision -- est_inv is a float slightly BELOW 2^32/q, so
// the estimate k' is floor(v/q) or one less (never above: the remainder stays non-negative) -- then v - k' q in [0,2q)
// and one conditional subtract finishes: 3 conversions/multiplies + 2 integer multiplies + 1 subtract step instead of
// four subtract steps.  Smaller moduli (top word too short for the estimate) take the four steps.
// Contract with the host (agx_ntt.cpp build_plan): est_inv != 0 only for q in [2^58, 2^60], so v < 16q <= 2^64 holds wherever the
// estimate path runs; the kernels that call this are the 16q-lazy ones (rb2_frame::EST requires LAZY16, legal for q <= 2^60 only).
// USE_EST: 1 = the caller has checked k.est_inv != 0 (quotient estimate), 0 = it has checked it is 0 (four steps), -1 = decide here
template <bool SEL, int USE_EST = -1>
__device__ __forceinline__ uint64_t reduce_final_est(uint64_t v, const bf_consts& k, const final_consts& f, bool lazy_out) {
    static_assert(SEL, "select-based conditional subtract only");
    if (USE_EST == 1 || (USE_EST == -1 && k.est_inv != 0.0f)) {   // wave-uniform
        const uint32_t kq = (uint32_t)((float)(uint32_t)(v >> 32) * k.est_inv);
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        u32x2 r = __builtin_bit_cast(u32x2, mad64(kq, (uint32_t)k.nq, v));      // v + k' * (2^64 - q), low word of -q
        r.y += kq * (uint32_t)(k.nq >> 32);                                      // ... and its high word
        const uint64_t r64 = __builtin_bit_cast(uint64_t, r);
        return lazy_out ? r64 : csub_select_c(r64, f.nq1);
    }
    v = csub_select_c(v, f.nq8);
    v = csub_select_c(v, k.nm);          // 4q
    if (lazy_out) return v;
    v = csub_select_c(v, f.nq2);
    return csub_select_c(v, f.nq1);
}

// ---------------------------------------------------------------------------------------
// q = 2^60 - c with 0 < c < 2^28 (the primes just below 2^60 that RNS users pick; every modulus of the plan must be
// of this form: arithmetic level 3).  The 16q-lazy forward transform with the tail-free schedule, and 2^60 = c (mod q)
// in place of the two operations that treat q as an opaque number:
//  * the mid-transform conditional subtract tests the SIGN BIT instead of comparing with 8q = 2^63 - 8c:
//    x >= 2^63 -> x - 8q = (x - 2^63) + 8c, else x stays.  A kept x lies below 2^63 = 8q + 8c rather than below 8q, so
//    the bounds carry a slack of 8c (q60c_tailfree: b q + e 8c); nothing passes 16q + 8c = 2^64 - 8c.
//  * the final reduction folds the top four bits: v = k 2^60 + r = r + k c (mod q).
// Same residues as the other forms at every stage, so the fully reduced outputs are identical.
// ---------------------------------------------------------------------------------------
struct q60c_tailfree {
    struct bound {
        int b, e;      // coefficients below b q + e 8c
    };
    // bound on the coefficients entering stage s (s = total: on the transform's outputs); inputs are < 4q
    static constexpr bound bound_in(int s, int total) {
        bound v{4, 0};
        for (int i = 0; i < s; ++i) {
            if (lazy16_tailfree::subtracts(i, total)) {
                // sign bit set: x - 8q < (b - 8) q + e 8c; clear: x < 2^63 = 8q + 8c
                v.b = v.b - 8 > 8 ? v.b - 8 : 8;
                v.e = v.e > 1 ? v.e : 1;
            }
            v.b += 4;      // x' = tx + Q~, y' = tx + 4q - Q~, Q~ < 4q
        }
        return v;
    }
    // every stage's inputs and the outputs stay within 16q + 8c = 2^64 - 8c, so no sum wraps and a set sign bit means x >= 2^63 > 8q
    static constexpr bool valid(int total) {
        for (int s = 0; s <= total; ++s) {
            const bound v = bound_in(s, total);
            if (v.b > 16 || v.e > 1) return false;
        }
        return lazy16_tailfree::valid(total);
    }
};

// x < 2^64 -> x - [x >= 2^63] 8q, below max(2^63, x - 8q): shift, mask and one multiply-add (8c < 2^31) instead of a 64-bit add,
// a 64-bit compare and two selects
__device__ __forceinline__ uint64_t csub_8q_q60c(uint64_t x, const bf_consts& k) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 v = __builtin_bit_cast(u32x2, x);
    uint32_t s = v.y >> 31;
    asm("" : "+v"(s));      // opaque: a known 0 / 1 factor turns the multiply-add back into a compare and selects
    v.y &= 0x7fffffffu;
    return mad64(s, k.c8, __builtin_bit_cast(uint64_t, v));
}

template <bool DO_CSUB>
__device__ __forceinline__ void ct_butterfly_q60c(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp, const bf_consts& k) {
    const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32), p0 = (uint32_t)wp, p1 = (uint32_t)(wp >> 32);
    const uint64_t tx = DO_CSUB ? csub_8q_q60c(x, k) : x;
    uint64_t c = mad64(p1, y1, (uint64_t)__umulhi(y0, p1));                  // one v_mov builds the {h,0} pair
    c = add64_32(c, __umulhi(y1, p0), k.one_b);
    const uint64_t xn = fold_product(tx, y, w, c, k);
    y = (tx << 1) + k.m - xn;                                               // tx + 4q - Q~
    x = xn;
}

// any v < 2^64 (the transform's outputs are below 16q + 8c) -> [0,q), or only below 2q for lazy outputs.  v = k 2^60 + r with
// k = v >> 60 <= 15 and r < 2^60; 2^60 = c (mod q), so v = r + k c (mod q), and with c < 2^28: k c < 15 2^28 < 2^32,
// r + k c < 2^60 + 2^32 < 2^61 - 2^29 < 2q.  One conditional subtract of q finishes (r + k c < 2^63: the sign test is exact).
// The fold itself: any x < 2^64 -> (x mod 2^60) + (x >> 60) c <= 2^60 - 1 + 15c, the same residue: shift, mask, one multiply-add.
// PIN (the butterflies of the skip form): the shifted word passes through an empty asm statement, as csub_8q_q60c's does -- no instruction, but the
// n = 4096 kernel is then allocated 111 VGPRs, as with the sign-bit subtract, instead of 115 (about 92 values are live either way).
template <bool PIN = false>
__device__ __forceinline__ uint64_t reduce_top4_q60c(uint64_t x, const bf_consts& k) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 r = __builtin_bit_cast(u32x2, x);
    uint32_t kq = r.y >> 28;
    if constexpr (PIN) asm("" : "+v"(kq));
    r.y &= 0x0fffffffu;
    return mad64(kq, k.c, __builtin_bit_cast(uint64_t, r));
}
__device__ __forceinline__ uint64_t reduce_final_q60c(uint64_t v, const bf_consts& k, const final_consts& f, bool lazy_out) {
    const uint64_t t = reduce_top4_q60c(v, k);
    return lazy_out ? t : csub_select_c(t, f.nq1);
}

// ---------------------------------------------------------------------------------------
// TWO-TWIDDLE form for the same class of moduli: six multiply-adds per butterfly, no quotient estimate.  The 124-bit product y w is never
// built; y = y0 + y1 2^32 meets a second twiddle wC = w 2^32 mod q (kept in the table slot where the other forms keep w'), so that
//   y w = y0 w + y1 wC (mod q).
// Both twiddles are split at bit 29 (wl = w mod 2^29, wh = w >> 29 < 2^31 because w < q < 2^60; wCl, wCh likewise):
//   hi = y0 wh + y1 wCh,   lo = y0 wl + y1 wCl,   y0 w + y1 wC = lo + hi 2^29 = lo + hl 2^29 + hh 2^61   (hl, hh: the words of hi)
// and 2^61 = 2c (mod q):  Q = lo + hl 2^29 + hh 2c = y w (mod q).  The whole right-hand side is ONE chain of v_mad_u64_u32 that lands on tx:
//   x' = tx + Q,   y' = tx + 8q - Q = 2 tx + 8q - x'.
// Coefficients travel between stages as arbitrary 64-bit words; every stage but the first brings x below 2^63 + 8c with the sign-bit
// subtract (csub_8q_q60c), the first one's inputs are below 4q.  q60c_fold_bounds proves that no partial sum wraps, for the whole class.
// (For c <= 2^27 half of those subtracts go: the skip form below, 7q in place of 8q.)
// reduce_final_q60c takes any 64-bit word, so the last stage and the output contract are those of the form above.
// ---------------------------------------------------------------------------------------
struct q60c_fold_bounds {
    typedef unsigned __int128 u128;
    static constexpr u128 two64 = (u128)1 << 64, w32 = 0xffffffffull;
    static constexpr u128 c_max = (1ull << 28) - 1, q_min = (1ull << 60) - (uint64_t)c_max, q_max = (1ull << 60) - 1;
    static constexpr u128 wh_max = (uint64_t)q_max >> 29, wl_max = (1ull << 29) - 1;      // halves of a twiddle below q
    static constexpr u128 hi_max = 2 * w32 * wh_max;                                         // y0 wh + y1 wCh
    static constexpr u128 lo_max = 2 * w32 * wl_max;                                         // y0 wl + y1 wCl
    static constexpr u128 Q_max = lo_max + w32 * ((u128)1 << 29) + w32 * 2 * c_max;          // lo + hl 2^29 + hh 2c, the largest c
    static constexpr u128 tx_max = ((u128)1 << 63) + 8 * c_max - 1, tx_max_c1 = ((u128)1 << 63) + 8 - 1;      // after csub_8q_q60c, the largest c and c = 1; a first-stage input is below 4q < 2^62
    static_assert(wh_max < ((u128)1 << 31), "the high half of a twiddle fits 31 bits");
    static_assert(hi_max < two64, "hi fits 64 bits");
    static_assert(tx_max + Q_max < two64, "x' = tx + Q does not wrap (every partial sum of the chain is below this one)");
    static_assert(Q_max <= 8 * q_min, "y' = tx + 8q - Q is not negative");
    static_assert(tx_max + 8 * q_min < two64 && tx_max_c1 + 8 * q_max < two64, "y' <= tx + 8q = 2^64 - 1 for every c");
};

// RARE last subtract (rb_frame.hpp: kOptQ60cRareSub).  A transform's output leaves the fold as t = r + k c, r < 2^60, k <= 15 (reduce_top4_q60c), and the
// conditional subtract of q that finishes it acts only when t >= q = 2^60 - c.  With c < 2^28 the whole interval [q, 2^60 + 15c) has a high word of at
// least 0x0FFFFFFF, so ONE 32-bit compare of the high word flags every coefficient that needs the subtract (and some that do not: t in
// [0x0FFFFFFF 2^32, q), about 2^-28 of the residues).  The kernel ORs the flags of a wave into a scalar mask and runs the subtract, over every register,
// only in a wave whose mask is not zero; the results are word for word those of a subtract per coefficient.
constexpr uint32_t kQ60cTailHi = 0x0fffffffu;
struct q60c_tail_bounds {
    typedef unsigned __int128 u128;
    using F = q60c_fold_bounds;
    static constexpr u128 t_max = ((u128)1 << 60) - 1 + 15 * F::c_max;      // after reduce_top4_q60c, the largest c of the class
    static_assert(15 * F::c_max < ((u128)1 << 32), "k c fits a word: the fold cannot carry t past bit 61");
    static_assert(t_max < ((u128)1 << 63), "the sign test of the cold block's csub_select_c is exact");
    static_assert((F::q_min >> 32) >= kQ60cTailHi, "t >= q implies hi32(t) >= 0x0FFFFFFF, for every c of the class (q falls as c grows)");
    static_assert((((u128)kQ60cTailHi << 32) - 1) < F::q_min, "a coefficient that is not flagged is below q");
};
// wave mask of the lanes whose t may need the last subtract: one VOPC compare per output that writes an SGPR pair.  The optimiser widens the test of the
// high word to the same predicate on the whole word, t >= 0x0FFFFFFF 2^32 (v_cmp_lt_u64); forced to 32 bits through the compare intrinsic it measured the same
// energy, and the headline sessions that decided this form were run on the one below (profiles/r18_final_subtract_bench_runs.txt)
__device__ __forceinline__ uint64_t q60c_tail_flag(uint64_t t) { return __builtin_amdgcn_ballot_w64((uint32_t)(t >> 32) >= kQ60cTailHi); }

// 2^29 as opaque_one() gives 1: the factor of hl stays a multiply-add
__device__ __forceinline__ uint32_t opaque_two29() {
    uint32_t v;
    asm("s_mov_b32 %0, 0x20000000" : "=s"(v));
    return v;
}

// SKIP form of the same butterfly for c <= kQ60cSkipMaxC = 2^27: the lazy-range constant is 7q (y' = tx + 7q - Q), and x is reduced by its top four
// bits (reduce_top4_q60c: the same three instructions as the sign-bit subtract) on every SECOND stage only; the stages between reduce nothing.
//   reducing stage, any 64-bit x:   tx <= 2^60 - 1 + 15c,   x' = tx + Q and y' = tx + 7q - Q are at most tx + 7q = 8q + 16c - 1 = 2^63 + 8c - 1
//   the stage behind it, tx = x:    x' and y' are at most 15q + 16c - 1 = 2^64 - q - 1
// because Q <= 7q for this class (lo + hl 2^29 < 6q, hh 2c < 2^33 c <= 2^60; 7q is also what keeps y' from going negative).  2 tx may pass 2^64 in
// y' = 2 tx + 7q - x'; the value itself lies in [0, 2^64), so arithmetic mod 2^64 returns it.  y-inputs may be any 64-bit word, as above, and so may the
// inputs of stage 0, which reduces.  q60c_skip_bounds proves it for the whole class; the schedule says which stages reduce.
struct q60c_skip_schedule {
    static constexpr bool reduces(int s) { return (s & 1) == 0; }
    // stage 0 takes any word, and no unreduced stage follows another: the proof covers one reduced stage plus one unreduced stage.  The last stage
    // may be either: reduce_final_q60c takes any word.
    static constexpr bool valid(int total) {
        for (int s = 1; s < total; ++s)
            if (!reduces(s) && !reduces(s - 1)) return false;
        return total >= 1 && reduces(0);
    }
};
struct q60c_skip_bounds {
    typedef unsigned __int128 u128;
    using F = q60c_fold_bounds;
    static constexpr u128 two64 = F::two64, w32 = F::w32;
    static constexpr u128 c_max = kQ60cSkipMaxC, q_min = (1ull << 60) - (uint64_t)c_max;
    static constexpr u128 Q_max = F::lo_max + w32 * ((u128)1 << 29) + w32 * 2 * c_max;      // lo + hl 2^29 + hh 2c; grows with c, while q falls: the largest c decides
    static constexpr u128 r_max = ((u128)1 << 60) - 1 + 15 * c_max;                          // after reduce_top4_q60c
    static constexpr u128 out1_max = r_max + 7 * q_min;                                      // x', y' of a reducing stage (Q <= 7q): 2^63 + 8c - 1, largest at the largest c
    static_assert(c_max < ((u128)1 << 28), "a subclass of the moduli of q60c_fold_bounds: hi and the halves of a twiddle are bounded there");
    static_assert(15 * c_max < ((u128)1 << 32), "the fold's product fits a word");
    static_assert(Q_max <= 7 * q_min, "y' = tx + 7q - Q is not negative, on either kind of stage");
    static_assert(out1_max == ((u128)1 << 63) + 8 * c_max - 1, "8q + 16c - 1");
    static_assert(r_max + Q_max < two64, "reducing stage: x' does not wrap (every partial sum of the chain is below this one)");
    static_assert(out1_max + Q_max < two64, "the stage behind it: x' does not wrap (every partial sum of the chain is below this one)");
    static_assert(out1_max + 7 * q_min < two64, "... and y' <= tx + 7q = 15 2^60 + c - 1 (grows with c) stays below 2^64");
};

// FORM 0 / 1: lazy-range constant 8q (k.mfold), x as it comes / after the sign-bit subtract.  FORM 2 / 3: the skip form, lazy-range constant 7q,
// x after the reduction by its top four bits / as it comes.
template <int FORM>
__device__ __forceinline__ void ct_butterfly_q60c_fold(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wC, const bf_consts& k) {
    static_assert(FORM >= 0 && FORM <= 3, "no such form");
    const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32);
    const uint32_t wl = (uint32_t)w, wh = (uint32_t)(w >> 32), wCl = (uint32_t)wC, wCh = (uint32_t)(wC >> 32);      // the slot holds the halves a word each
    const uint64_t tx = FORM == 1 ? csub_8q_q60c(x, k) : FORM == 2 ? reduce_top4_q60c<true>(x, k) : x;
    const uint64_t hi = mad64(y1, wCh, mul64(y0, wh));
    uint64_t xn = keep64(mad64(y0, wl, tx));      // pinned: left free, the sum is reassociated into a chain from zero plus a 64-bit add of tx
    xn = mad64(y1, wCl, xn);
    xn = mad64((uint32_t)hi, k.p29, xn);      // a visible 2^29 would become shifts and a carry pair
    xn = mad64((uint32_t)(hi >> 32), k.c2, xn);
    y = (tx << 1) + k.mfold - xn;                                           // tx + 8q - Q (skip form: 7q)
    x = xn;
}

// w*d - c*q (mod 2^64) with the quotient estimate of the chosen arithmetic:
// exact -> [0,2q), fast -> [0,4q); d may be any 64-bit value
template <bool FAST>
__device__ __forceinline__ uint64_t mul_shoup_form(uint64_t d, uint64_t w, uint64_t wp, const bf_consts& k) {
    const uint32_t d0 = (uint32_t)d, d1 = (uint32_t)(d >> 32), p0 = (uint32_t)wp, p1 = (uint32_t)(wp >> 32);
    uint64_t c;
    if constexpr (FAST) {
        c = mad64(p1, d1, (uint64_t)__umulhi(d0, p1));
        c = add64_32(c, __umulhi(d1, p0), k.one_b);
    } else {
        const uint32_t t = __umulhi(d0, p0);
        const uint64_t m1 = add64_32(mul64(p1, d0), t, k.one_a);
        const uint64_t m2 = add64_32(mul64(p0, d1), (uint32_t)m1, k.one_b);
        c = add64_32(mul64(p1, d1), (uint32_t)(m1 >> 32), k.one_a);
        c = add64_32(c, (uint32_t)(m2 >> 32), k.one_b);
    }
    return fold_product(0, d, w, c, k);
}

// Gentleman-Sande butterfly of the inverse transform, coefficients in [0,m)
// (m = 2q exact / 4q fast): x' = x + y - [x+y >= m] m,  y' = w (x - y + m) lazily reduced.
template <bool FAST, bool SEL = false>
__device__ __forceinline__ void gs_butterfly_form(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp, const bf_consts& k) {
    const uint64_t s = x + y;
    const uint64_t d = x + k.m - y;
    if constexpr (FAST) x = SEL ? csub_select(s, k) : csub_sign(s, k);
    else x = csub(s, k.m);
    y = mul_shoup_form<FAST>(d, w, wp, k);
}

// last inverse stage with n^-1 folded in: x' = (x + y) n^-1, y' = (x - y) w n^-1
template <bool FAST>
__device__ __forceinline__ void gs_last_form(uint64_t& x, uint64_t& y, uint64_t ninv, uint64_t ninv_p,
                                             uint64_t w1n, uint64_t w1n_p, const bf_consts& k) {
    const uint64_t s = x + y;
    const uint64_t d = x + k.m - y;
    x = mul_shoup_form<FAST>(s, ninv, ninv_p, k);
    y = mul_shoup_form<FAST>(d, w1n, w1n_p, k);
}

// 16q-lazy Gentleman-Sande butterflies (q <= 2^60, so 16q <= 2^64).  y' = w d is below 4q whatever d is, so
// only the sums grow: B is the compile-time bound, in units of q, that both inputs share (4, 8 or 16 -- a
// butterfly's two inputs always have the same history).  Inputs at 16q are first brought below 8q; then
// x' = x + y < 2b q <= 16q and d = x - y + b q in (0, 16q).  The caller tracks the bounds (gs_bound).
template <bool SEL>
__device__ __forceinline__ uint64_t csub_8q(uint64_t v, const final_consts& f) {
    return SEL ? csub_select_c(v, f.nq8) : csub_sign_c(v, f.q8, f.nq8);
}
// bound of register r entering stage s of a pass whose registers all start below B0*q: the X output of a
// stage doubles its (reduced) input bound, the Y output is below 4q
constexpr int gs_bound(int B0, int s, int r) {
    if (s == 0) return B0;
    if ((r >> (s - 1)) & 1) return 4;
    const int b = gs_bound(B0, s - 1, r);
    return 2 * (b == 16 ? 8 : b);
}
template <int B, bool SEL>
__device__ __forceinline__ void gs_butterfly_lazy16(uint64_t& x, uint64_t& y, uint64_t w, uint64_t wp, const bf_consts& k, const final_consts& f) {
    static_assert(B == 4 || B == 8 || B == 16, "bounds are 4q, 8q or 16q");
    if constexpr (B == 16) {
        x = csub_8q<SEL>(x, f);
        y = csub_8q<SEL>(y, f);
    }
    const uint64_t s = x + y;
    const uint64_t d = x + (B == 4 ? k.m : f.q8) - y;
    y = mul_shoup_form<true>(d, w, wp, k);
    x = s;
}
template <int B, bool SEL>
__device__ __forceinline__ void gs_last_lazy16(uint64_t& x, uint64_t& y, uint64_t ninv, uint64_t ninv_p, uint64_t w1n, uint64_t w1n_p,
                                               const bf_consts& k, const final_consts& f) {
    if constexpr (B == 16) {
        x = csub_8q<SEL>(x, f);
        y = csub_8q<SEL>(y, f);
    }
    const uint64_t s = x + y;
    const uint64_t d = x + (B == 4 ? k.m : f.q8) - y;
    x = mul_shoup_form<true>(s, ninv, ninv_p, k);
    y = mul_shoup_form<true>(d, w1n, w1n_p, k);
}

// [0,m) -> [0,q) after the inverse transform
template <bool FAST, bool SEL = false>
__device__ __forceinline__ uint64_t reduce_final_inv(uint64_t v, const bf_consts& k, const final_consts& f) {
    if constexpr (FAST && SEL) {
        v = csub_select_c(v, f.nq2);
        return csub_select_c(v, f.nq1);
    } else if constexpr (FAST) {
        v = csub_sign_c(v, f.q2, f.nq2);
        return csub_sign_c(v, f.q1, f.nq1);
    } else {
        return csub(v, k.q);
    }
}

}  // namespace agx
