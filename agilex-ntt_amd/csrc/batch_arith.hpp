// batch_arith.hpp -- the per-word steps of agx_ntt_batch_encode and agx_ntt_batch_decode (SIMD batching of BFV / BGV: a vector of n slots modulo a prime
// t = 1 (mod 2n) <-> the plaintext polynomial that takes those values at the roots psi^{e_j}), beside bfv_conv_arith.hpp, whose Shoup product it uses.
// Compiles for the device (batch_kernels.hpp) and for the host (tests/batch_selftest.cpp runs this same text against unsigned __int128): no HIP header is
// needed on the host.  include/agx_ntt.h has the definition; host_math.hpp (batch_image) builds the two index tables.
//
//   batch_reduce    any 64-bit z -> z mod t in [0, t): bfv_shoup by the constant 1, whose quotient one_p = floor(2^64 / t) the handle keeps; the product
//                   z - floor(z one_p / 2^64) t lies in [0, 2t) for any z and any t with 2t < 2^64 (bfv_conv_arith.hpp), one subtraction ends it.
//   batch_source    the word a permuted word e = frame n + w comes from (or, for the scattered-write twin, goes to): frame n + idx, idx the table's entry
//                   for w.  The entry is masked to [0, n): the tables
//                   are permutations of [0, n) built on the host, never data, and the mask keeps the address inside the frame whatever they hold.
#pragma once
#include "bfv_conv_arith.hpp"

namespace agx {

AGX_HD uint64_t batch_reduce(uint64_t z, uint64_t one_p, uint64_t t) { return bfv_shoup(z, 1, one_p, t); }

AGX_HD uint64_t batch_source(uint64_t e, uint32_t log_n, uint32_t idx) {
    const uint64_t mask = (1ull << log_n) - 1;
    return (e & ~mask) | (idx & mask);
}

}  // namespace agx
