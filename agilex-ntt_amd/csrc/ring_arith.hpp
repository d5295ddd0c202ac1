// ring_arith.hpp -- the per-word arithmetic of agx_ntt_add / _sub / _negate / _add_galois / _tensor: lazy inputs in [0, 4q), fully reduced outputs.
// Compiles for the device (ring_kernels.hpp) and for the host (tests/ring_selftest.cpp runs this same text against unsigned __int128 %), as
// inner_reduce.hpp does and on top of it: no HIP header is needed on the host.
//
// Ranges, for any odd q < 2^62 (4q < 2^64, so every input word is what it says).
//   ring_reduce   [0, 4q) -> [0, q): two conditional subtracts (2q, then q).
//   ring_add      x + y < 2q < 2^63 for reduced x, y: one conditional subtract.
//   ring_sub      x + q - y lies in (0, 2q): one conditional subtract.
//   ring_neg      q - x for reduced x != 0, and 0 for x = 0 (q - 0 = q is not reduced).
//   ring_tensor   c_0 = a_0 b_0, c_2 = a_1 b_1: one product of reduced operands (below 2^124) through acc_mul_add and acc_reduce -- instruction for
//                 instruction mul_mod_barrett (modarith.hpp), which is that pair for a sum of one.  c_1 = a_0 b_1 + a_1 b_0: two products in ONE 128-bit
//                 sum (below 2^125, far inside the sixteen that inner_reduce.hpp's range argument admits) and ONE reduction of the cross term.
//                 The three-product form (a_0 + a_1)(b_0 + b_1) - a_0 b_0 - a_1 b_1 on unreduced 128-bit products was built and measured
//                 (profiles/r12_ring_ops.md): 3 ... 4 % faster at n = 16384, inside the four-product form's run-to-run spread at n = 4096; deleted.
#pragma once
#include "inner_reduce.hpp"

namespace agx {

AGX_HD uint64_t ring_csub(uint64_t v, uint64_t m) { return v >= m ? v - m : v; }
AGX_HD uint64_t ring_reduce(uint64_t v, uint64_t q, uint64_t q2) { return ring_csub(ring_csub(v, q2), q); }      // q2 = 2q

AGX_HD uint64_t ring_add(uint64_t a, uint64_t b, uint64_t q, uint64_t q2) { return ring_csub(ring_reduce(a, q, q2) + ring_reduce(b, q, q2), q); }
AGX_HD uint64_t ring_sub(uint64_t a, uint64_t b, uint64_t q, uint64_t q2) { return ring_csub(ring_reduce(a, q, q2) + q - ring_reduce(b, q, q2), q); }
AGX_HD uint64_t ring_neg(uint64_t a, uint64_t q, uint64_t q2) {
    const uint64_t x = ring_reduce(a, q, q2);
    return x ? q - x : 0;
}

// a x b mod q for reduced a, b
AGX_HD uint64_t ring_mul(uint64_t a, uint64_t b, uint64_t q, uint64_t mu_hi, uint64_t mu_lo) {
    acc128 s;
    acc_mul_add(s, a, b);
    return acc_reduce(s, q, mu_hi, mu_lo);
}

// (c0, c1, c2) = (a0 b0, a0 b1 + a1 b0, a1 b1) mod q; inputs in [0, 4q); {mu_hi, mu_lo} = floor(2^128 / q)
AGX_HD void ring_tensor(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1, uint64_t q, uint64_t mu_hi, uint64_t mu_lo, uint64_t& c0, uint64_t& c1, uint64_t& c2) {
    const uint64_t q2 = q << 1;
    a0 = ring_reduce(a0, q, q2), a1 = ring_reduce(a1, q, q2), b0 = ring_reduce(b0, q, q2), b1 = ring_reduce(b1, q, q2);
    c0 = ring_mul(a0, b0, q, mu_hi, mu_lo);
    acc128 cross;
    acc_mul_add(cross, a0, b1);
    acc_mul_add(cross, a1, b0);
    c1 = acc_reduce(cross, q, mu_hi, mu_lo);
    c2 = ring_mul(a1, b1, q, mu_hi, mu_lo);
}

}  // namespace agx
