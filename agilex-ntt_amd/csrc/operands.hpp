// operands.hpp -- the pure integer predicates behind the argument rules of include/agx_ntt.h section (3): does a frame layout fit, does
// it overlap itself, do two frame sets or two dense ranges touch.  No HIP, no plan: tests/operands_selftest.cpp checks them on a CPU.
// A frame set has num_primes x batch frames of n words; frame (p, b) starts p prime_stride + b poly_stride words after the base.
// Addresses are bytes (uintptr_t), everything else is counted in 8-byte words.
// Why nothing below overflows: callers ask layout_fits first and keep batch below 2^63 (the grid limit is 2^31 - 1).  Then (P-1) prime_stride,
// (B-1) poly_stride and their sum with n are at most 2^60; frames_touch gets a delta below the extent (partial_overlap) or 0 (self_overlap), so
// |delta + dp prime_stride + db poly_stride| <= 3 * 2^60; layout_fits works in 128 bits; ranges_touch subtracts the smaller address from the larger.
#pragma once
#include <cstdint>

namespace agx {

// Are both strides >= 0 and is the extent (P-1) prime_stride + (B-1) poly_stride + n at most 2^60 words (2^63 bytes: every byte offset from the
// base fits a signed 64-bit integer)?  An empty set has no extent.
inline bool layout_fits(uint32_t n, uint32_t num_primes, uint64_t batch, int64_t prime_stride, int64_t poly_stride) {
    if (prime_stride < 0 || poly_stride < 0) return false;
    if (num_primes == 0 || batch == 0) return true;
    using u128 = unsigned __int128;      // (2^32)(2^63) + (2^64)(2^63) + 2^32 < 2^128
    return (u128)(num_primes - 1) * (u128)prime_stride + (u128)(batch - 1) * (u128)poly_stride + n <= (u128)1 << 60;
}

// Does any frame of set A touch a frame of set B = A shifted by delta elements?  Frame (p, b) lies at base + p prime_stride + b poly_stride,
// n elements long; frames i of A and j of B touch iff |delta + dp prime_stride + db poly_stride| < n for their index differences
// (dp, db).  skip_self excludes (dp, db) = (0, 0) when delta = 0: a frame does not collide with itself.
inline bool frames_touch(int64_t delta, bool skip_self, uint32_t n, uint32_t num_primes, uint64_t batch, int64_t prime_stride, int64_t poly_stride) {
    const int64_t P = (int64_t)num_primes, B = (int64_t)batch;
    for (int64_t dp = -(P - 1); dp <= P - 1; ++dp) {
        const int64_t base = delta + dp * prime_stride;
        const bool self_row = skip_self && dp == 0;
        if (poly_stride == 0 || B == 1) {
            if (self_row) {
                if (B > 1) return true;      // poly_stride 0: frames (p, 0) and (p, 1) are the same words
                continue;
            }
            if (base > -(int64_t)n && base < (int64_t)n) return true;
            continue;
        }
        // db closest to -base / poly_stride, within [-(B-1), B-1]: try the two neighbours of the quotient
        int64_t d0 = -base / poly_stride;
        for (int64_t db = d0 - 1; db <= d0 + 1; ++db) {
            const int64_t dbc = db < -(B - 1) ? -(B - 1) : db > B - 1 ? B - 1 : db;
            if (self_row && dbc == 0) continue;
            const int64_t v = base + dbc * poly_stride;
            if (v > -(int64_t)n && v < (int64_t)n) return true;
        }
    }
    return false;
}

// Do two frame sets of the same shape, at byte addresses a and b, overlap without being the same set?  Identical bases are in place
// (legal: a workgroup reads its frame before it writes it); otherwise NO frame of one may touch any frame of the other, because
// workgroups run in any order (include/agx_ntt.h: AGX_ERR_BAD_ARGUMENT "overlapping in/out").  Interleaved layouts whose frames do not
// touch (out = in + n with poly_stride = 2n) are legal and pass.
inline bool partial_overlap(uintptr_t a, uintptr_t b, uint32_t n, uint32_t num_primes, uint64_t batch, int64_t prime_stride, int64_t poly_stride) {
    if (a == b || batch == 0) return false;
    const int64_t delta = b > a ? (int64_t)((b - a) / 8) : -(int64_t)((a - b) / 8);      // words (both 8-byte aligned), magnitude < 2^61
    const int64_t extent = (int64_t)(num_primes - 1) * prime_stride + (int64_t)(batch - 1) * poly_stride + (int64_t)n;
    if (delta >= extent || -delta >= extent) return false;      // disjoint ranges
    return frames_touch(delta, false, n, num_primes, batch, prime_stride, poly_stride);
}

// Does one frame set overlap itself (two distinct frames (p, b) != (p', b') touch)?  Two workgroups would then transform the same words
// in place, under different moduli for dp != 0: garbage.  The dense [prime][batch][n] layout and the [poly][prime][n] layout answer in
// O(1) (no loop on the latency path); anything else takes frames_touch's closest-db search with delta = 0.
inline bool self_overlap(uint32_t n, uint32_t num_primes, uint64_t batch, int64_t prime_stride, int64_t poly_stride) {
    if (batch == 0 || (num_primes == 1 && batch == 1)) return false;
    const int64_t N = (int64_t)n, P = (int64_t)num_primes, B = (int64_t)batch;
    // prime-major: batches of one prime are n apart, primes clear the whole batch
    if ((B == 1 || poly_stride >= N) && (P == 1 || prime_stride >= (B - 1) * poly_stride + N)) return false;
    // poly-major: primes of one polynomial are n apart, polynomials clear every prime
    if ((P == 1 || prime_stride >= N) && (B == 1 || poly_stride >= (P - 1) * prime_stride + N)) return false;
    return frames_touch(0, true, n, num_primes, batch, prime_stride, poly_stride);
}

// Do the dense ranges of a_words words at byte address a and of b_words words at b share a byte?  An empty range touches nothing, and
// a range may end at the top of the address space: no end address is ever formed.
inline bool ranges_touch(uintptr_t a, uint64_t a_words, uintptr_t b, uint64_t b_words) {
    if (a_words == 0 || b_words == 0) return false;
    return a <= b ? (b - a) / 8 < a_words : (a - b) / 8 < b_words;
}

// The buffer rule of the calls that bring xq (qwords words) down by xp (pwords words) through a scratch of pwords words into out (qwords words):
// agx_ntt_basis_mod_down, and agx_ntt_rescale with xq = slabs 0 .. P-2 of x and xp = its last slab.  Dense sets, one range each.
//   out IS xq (in place) or touches nothing of it;
//   out never touches xp or the scratch, the scratch never xq: several workgroups per frame read the scratch while others already write out, and
//   the first launch reads xp;
//   the scratch IS xp (the caller gives those slabs up) or does not touch it.
inline bool down_buffers_ok(uintptr_t xq, uint64_t qwords, uintptr_t xp, uint64_t pwords, uintptr_t out, uintptr_t scratch) {
    if (out != xq && ranges_touch(out, qwords, xq, qwords)) return false;
    if (ranges_touch(out, qwords, xp, pwords) || ranges_touch(out, qwords, scratch, pwords) || ranges_touch(scratch, pwords, xq, qwords)) return false;
    return scratch == xp || !ranges_touch(scratch, pwords, xp, pwords);
}

// The buffer rule of the calls that transform x (x_words words) into a scratch of as many words and stream out (out_words words) from it:
// agx_ntt_basis_quotient, agx_ntt_plain_scale_down / _reduce, agx_ntt_ckks_decode from NTT form and agx_ntt_batch_decode.  Dense sets, one range each.
//   the scratch IS x (the plan's inverse -- batch_decode's forward -- then runs in place, as agx_ntt_inverse may) or touches none of it: every
//   workgroup of the transform reads its frame of x before it writes the scratch's, but no other frame's;
//   out touches neither: the streaming kernel reads the scratch while other workgroups already write out, and the first launch reads x.
inline bool scratch_buffers_ok(uintptr_t x, uint64_t x_words, uintptr_t scratch, uintptr_t out, uint64_t out_words) {
    if (scratch != x && ranges_touch(scratch, x_words, x, x_words)) return false;
    return !ranges_touch(out, out_words, x, x_words) && !ranges_touch(out, out_words, scratch, x_words);
}

}  // namespace agx
