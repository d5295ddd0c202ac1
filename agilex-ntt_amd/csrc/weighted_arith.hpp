// weighted_arith.hpp -- the per-word finish of agx_ntt_keyswitch_accumulate_decomposed and agx_ntt_mul_add_galois: out = (old' + w' t) mod q, with t
// already reduced (the inner product's word, or the gathered operand b reduced), w and old anywhere in [0, 4q), x' = x mod q.
// Compiles for the device (weighted_kernels.hpp) and for the host (tests/weighted_selftest.cpp runs this same text against unsigned __int128 %), as
// ring_arith.hpp does and on top of it: no HIP header is needed on the host.
//
// Range argument, for any odd q < 2^62 (4q < 2^64, so every input word is what it says).
//   w' = ring_reduce(w) and old' = ring_reduce(old) lie in [0, q); t < q is the caller's promise (acc_reduce's output, or ring_reduce's).
//   w' t <= (q - 1)^2 < 2^124, formed by acc_mul_add into an empty {hi, lo} pair: no carry is lost.  Adding old' < 2^62 gives
//   w' t + old' < 2^124 + 2^62 < 2^128: the carry out of lo goes into hi, and hi < 2^60 + 1 cannot wrap.
//   acc_reduce admits ANY 128-bit value (inner_reduce.hpp: the remainder before the two conditional subtracts lies in [0, 4q)), so ONE reduction of the
//   pair is exact and fully reduced.  This is one more reduction per output word than the un-weighted inner product, and none per term.
//   Without a weight (w = 1): old' + t < 2q < 2^63, one conditional subtract, no product.  Without either: t itself.
#pragma once
#include "ring_arith.hpp"

namespace agx {

// (old' + w' t) mod q; t < q; w, old in [0, 4q); {mu_hi, mu_lo} = floor(2^128 / q)
AGX_HD uint64_t weighted_mul_add(uint64_t w, uint64_t t, uint64_t old, uint64_t q, uint64_t q2, uint64_t mu_hi, uint64_t mu_lo) {
    acc128 s;
    acc_mul_add(s, ring_reduce(w, q, q2), t);
    const uint64_t o = ring_reduce(old, q, q2);
    s.lo += o;
    s.hi += s.lo < o ? 1u : 0u;
    return acc_reduce(s, q, mu_hi, mu_lo);
}

// the finish of one word: has_w / has_old say whether a weight and an old word take part (wave-uniform in the kernels); w and old are not looked at otherwise
AGX_HD uint64_t weighted_finish(uint64_t t, bool has_w, uint64_t w, bool has_old, uint64_t old, uint64_t q, uint64_t q2, uint64_t mu_hi, uint64_t mu_lo) {
    if (has_w) return weighted_mul_add(w, t, has_old ? old : 0, q, q2, mu_hi, mu_lo);
    return has_old ? ring_csub(ring_reduce(old, q, q2) + t, q) : t;
}

}  // namespace agx
