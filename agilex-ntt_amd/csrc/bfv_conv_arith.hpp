// bfv_conv_arith.hpp -- the per-word steps that agx_ntt_basis_extend_exact (Shenoy-Kumaresan) and agx_ntt_basis_extend_mont (BEHZ: FastBConv_m~ followed
// by the small Montgomery reduction) add to the fast base conversion, all with wave-uniform constants.  Compiles for the device (basis_aux_coeff_kernel of
// basis_coeff_kernels.hpp) and for the host (tests/bfv_conv_selftest.cpp runs this same text against unsigned __int128), as moddown_arith.hpp does: no HIP header
// is needed on the host.
//
// With D = prod of the sources q_i, D_i = D / q_i, the auxiliary prime m, V = sum_i y_i D_i and centre(a) = a for a <= (m - 1) / 2, a - m above:
//   exact   y_i = x_i D_i^-1 mod q_i,      alpha = centre((V - r) D^-1 mod m),   out_j = (V - alpha D) mod q_j;
//   mont    y_i = x_i m D_i^-1 mod q_i,    alpha = centre(-V D^-1 mod m),        out_j = (V + alpha D) m^-1 mod q_j.
// Both are ONE body with two constant sets {k, M_ji, c_j}: alpha = centre((V - r) k mod m) and out_j = (sum_i y_i M_ji) - alpha c_j mod q_j, with
//   exact   k = D^-1 mod m,    M_ji = D_i mod q_j,         c_j = D mod q_j,          r the auxiliary word;
//   mont    k = -D^-1 mod m,   M_ji = D_i m^-1 mod q_j,    c_j = -D m^-1 mod q_j,    r = 0.
// Ranges, for any odd modulus below 2^62, tiny ones included (a Shoup product w y - floor(w' y / 2^64) q lies in [0, 2q) for ANY 64-bit y and any q:
// w' = floor(w 2^64 / q) makes the quotient estimate exact or one short, whatever the ratio y / q).
//   bfv_reduce_lazy   a word in [0, 4m) (4m < 2^64) -> [0, m): two conditional subtracts.
//   bfv_shoup         any 64-bit y, w in [0, q) with its quotient -> w y mod q in [0, q): the lazy product and one conditional subtract.
//   bfv_alpha         vm, r in [0, m): vm - r where that is not negative, vm - r + m in (0, m) where it is; then one Shoup product by k: the result in [0, m).
//   bfv_centre        a in [0, m), m odd: |centre(a)| = a for a <= (m - 1) / 2 and m - a in [1, (m - 1) / 2] above, where *negative is set.  a = (m - 1) / 2
//                     stays positive and a = (m + 1) / 2 becomes -(m - 1) / 2: the two edges.  The magnitude is below 2^61.
//   bfv_correct       acc in [0, 2q_j) as basis_accumulate leaves it, mag in [0, (m - 1) / 2] (a residue of ANOTHER modulus: bfv_shoup takes it to
//                     [0, q_j)): acc is brought below q_j, then acc - p where alpha is positive (+ q_j where that is negative) and acc + p, less q_j from
//                     q_j on, where alpha is negative; no sum passes 2q_j < 2^63.  The result is fully reduced.
#pragma once
#include "inner_reduce.hpp"      // AGX_HD, umulhi64

namespace agx {

AGX_HD uint64_t bfv_reduce_lazy(uint64_t v, uint64_t m) {
    const uint64_t m2 = m << 1;
    v = v >= m2 ? v - m2 : v;
    return v >= m ? v - m : v;
}

AGX_HD uint64_t bfv_shoup(uint64_t y, uint64_t w, uint64_t wp, uint64_t q) {
    const uint64_t p = w * y - umulhi64(y, wp) * q;
    return p >= q ? p - q : p;
}

AGX_HD uint64_t bfv_alpha(uint64_t vm, uint64_t r, uint64_t k, uint64_t kp, uint64_t m) { return bfv_shoup(vm - r + (vm < r ? m : 0), k, kp, m); }

AGX_HD uint64_t bfv_centre(uint64_t a, uint64_t m, bool* negative) {
    *negative = a > (m >> 1);
    return *negative ? m - a : a;
}

AGX_HD uint64_t bfv_correct(uint64_t acc, uint64_t mag, bool negative, uint64_t c, uint64_t cp, uint64_t q) {
    const uint64_t v = acc >= q ? acc - q : acc, p = bfv_shoup(mag, c, cp, q);
    if (negative) {
        const uint64_t s = v + p;
        return s >= q ? s - q : s;
    }
    return v - p + (v < p ? q : 0);
}

}  // namespace agx
