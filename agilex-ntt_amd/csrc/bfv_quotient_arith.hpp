// bfv_quotient_arith.hpp -- the per-word steps of agx_ntt_basis_quotient (BFV's divide-and-return: the fast floor of t X / Q on Bsk and the Shenoy-Kumaresan
// return to Q, in one coefficient-domain kernel), beside those of bfv_conv_arith.hpp, which it also uses.  Compiles for the device
// (basis_quotient_kernel of basis_coeff_kernels.hpp) and for the host (tests/bfv_quotient_selftest.cpp runs this same text against unsigned __int128).
//
// With Q = prod q_i over the L primes of Q, Q_i = Q / q_i, B = prod b_j over the K primes of B, B_j = B / b_j and m the auxiliary prime, the scaled
// inverses hand the kernel, per coefficient (a_. the coefficient forms of the input slabs, reduced),
//   y_i = t a_i Q_i^-1 mod q_i  in [0, q_i),    s_j = t a_j Q^-1 B_j^-1 mod b_j  in [0, b_j),    s_m = t a_m Q^-1 mod m  in [0, m),
// and with V = sum_i y_i Q_i the contract's words are
//   f_j = (t a_j - V) Q^-1 mod b_j,    z_j = f_j B_j^-1 mod b_j = s_j - sum_i y_i (q_i^-1 B_j^-1 mod b_j)  mod b_j     since Q^-1 Q_i = q_i^-1,
//   f_m = s_m - sum_i y_i (q_i^-1 mod m)  mod m,    W mod m = sum_j z_j (B_j mod m),    alpha = centre((W - f_m) B^-1 mod m),
//   out_i = sum_j z_j (B_j mod q_i) - alpha (B mod q_i)  mod q_i.
// The z_j and f_m are residues in [0, b_j) and [0, m): W = sum_j z_j B_j is an integer formula in them, so their representative matters.  The sums over
// i are accumulated per y_i as it is read, so no y_i is kept: K accumulators, f_m's, and one y_i are live.
//   quot_accumulate   acc in [0, 2q), any 64-bit y (a residue of ANOTHER modulus), {c, cp} a word below q with its quotient: acc + c y mod q in [0, 2q).
//                     The Shoup product lies in [0, 2q) for any y and any q (bfv_conv_arith.hpp), the sum below 4q < 2^64, one conditional subtract
//                     of 2q.  This is basis_accumulate of modarith.hpp in text both compilers take.
//   quot_residue      s in [0, q), acc in [0, 2q): (s - acc) mod q in [0, q): acc is brought below q, then s - acc where that is not negative and
//                     s - acc + q in (0, q) where it is.
// alpha and the correction are bfv_alpha, bfv_centre and bfv_correct with k = B^-1 mod m, r = f_m and c_i = B mod q_i: the constants of the exact conversion.
#pragma once
#include "bfv_conv_arith.hpp"

namespace agx {

AGX_HD uint64_t quot_accumulate(uint64_t acc, uint64_t y, uint64_t c, uint64_t cp, uint64_t q, uint64_t q2) {
    const uint64_t s = acc + (c * y - umulhi64(y, cp) * q);
    return s >= q2 ? s - q2 : s;
}

AGX_HD uint64_t quot_residue(uint64_t s, uint64_t acc, uint64_t q) {
    const uint64_t a = acc >= q ? acc - q : acc;
    return s - a + (s < a ? q : 0);
}

}  // namespace agx
