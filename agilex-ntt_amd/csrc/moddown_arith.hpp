// moddown_arith.hpp -- the two per-word steps that AGX_RESCALE_ROUND adds to agx_ntt_basis_mod_down_mode, both with wave-uniform constants.
// Compiles for the device (moddown_round_rb2 of rb_kernels.hpp, moddown_coeff_round_kernel of basis_coeff_kernels.hpp) and for the host
// (tests/moddown_modes_selftest.cpp runs this same text against unsigned __int128), as ring_arith.hpp and weighted_arith.hpp do: no HIP header is
// needed on the host.
//
// With D = prod of the sources q_i, D_i = D / q_i, h = floor(D / 2) = (D - 1) / 2 (D is odd) and the plaintext modulus t of the basis:
//   y_i   = ((p_i t^-1 mod q_i) + (h mod q_i)) D_i^-1 mod q_i = y_i(floor) + c_i mod q_i,   c_i = h D_i^-1 mod q_i;
//   out_j = (a_j - (t mod q_j) ((V - h) mod q_j)) D^-1 mod q_j,  V = sum_i y_i D_i: the accumulator sum_i y_i (t D_i mod q_j) less hq_j = t h mod q_j.
// Ranges, for any odd modulus below 2^62.
//   moddown_round_y     y and c both in [0, q_i): y + c < 2 q_i < 2^63, one conditional subtract, the result the CANONICAL representative in [0, q_i) --
//                       V is an integer formula in the y_i, so their representative matters (as basis_scale's, modarith.hpp).
//   moddown_round_acc   acc in [0, 2q_j) as basis_accumulate leaves it, hq in [0, q_j): acc - hq where that is not negative, and acc - hq + q_j in
//                       (0, q_j) where it is.  The result stays in [0, 2q_j): what the forward passes and the coefficient-domain finish take today.
#pragma once
#include "inner_reduce.hpp"      // AGX_HD

namespace agx {

AGX_HD uint64_t moddown_round_y(uint64_t y, uint64_t c, uint64_t qi) {
    const uint64_t s = y + c;
    return s >= qi ? s - qi : s;
}

AGX_HD uint64_t moddown_round_acc(uint64_t acc, uint64_t hq, uint64_t q) { return acc - hq + (acc < hq ? q : 0); }

}  // namespace agx
