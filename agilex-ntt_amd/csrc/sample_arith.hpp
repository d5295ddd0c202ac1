// sample_arith.hpp -- the per-cell and per-word steps of agx_ntt_sample_uniform / _ternary / _cbd: the ChaCha20 block function (RFC 8439, section 2.3, 20
// rounds) as a counter-based generator, and the three ways its 64-bit candidates become coefficients.  Compiles for the device (sample_kernels.hpp) and for the
// host (tests/sample_selftest.cpp runs this same text against the RFC's vectors and a brute-force restatement), as plain_arith.hpp does: no HIP header is
// needed on the host.  include/agx_ntt.h states the definition; tests/sample_ref.py is its model in Python integers.
//
//   block(key, w12, w13, w14, w15): state words 0..3 the constants, 4..11 the key (little-endian words), 12..15 as given; o[0..15] the output.  The eight
//   candidates of a block are c_i = o[2i] | o[2i+1] << 32.  A cell is eight consecutive coefficients of one frame (c = j >> 3, W = min(8, n - 8c) words):
//   w12 = tag << 16 | c << 4 | k, w13 = the frame's number F, w14 / w15 = the low / high half of the nonce.
//   sample_uniform_cell  tag = the prime's index, k = 0, 1, ... the block counter: candidates masked to bitlen(q) bits are taken in order while below q; the
//                        r-th one accepted is word r of the cell; words still open after block 15 are 0.  It asks its source for block k only while words
//                        are open, and never for a block past 15: tests/sample_selftest.cpp drives the cap with a source that rejects everything.
//   sample_ternary       the first of the 32 two-bit fields of a candidate that is not 3 (0 -> 0, 1 -> +1, 2 -> -1; none: 0), without a branch: the fields
//                        that are not 3 are the non-zero fields of ~w, marked at their even bit by (m | m >> 1) & 0x5555...; bit 62 stands guard, so the count
//                        of trailing zeros is defined and a word of all ones reads its own last field, 3, whose value (f & 1) - (f >> 1) is 0 as well.
//   sample_cbd           popcount of the low eta bits of the low half less that of the high half: centred binomial, variance eta / 2, 1 <= eta <= 32.
//   sample_residue       a small signed value v, |v| <= 32, under a modulus, fully reduced: v for v >= 0, q + v otherwise.  Every modulus above 32 takes
//                        exactly that; one of the few admitted moduli up to 32 (5, 13, 17, 29: test plans) brings |v| below q first, by subtraction.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AGX_SAMPLE_HD __host__ __device__ __forceinline__
#define AGX_SAMPLE_UNROLL _Pragma("unroll")
#else
#define AGX_SAMPLE_HD inline
#define AGX_SAMPLE_UNROLL
#endif

namespace agx {

constexpr uint32_t kSampleMaxBlocks = 16;      // block counters 0 .. 15 of a uniform cell
constexpr uint32_t kSampleSmallTag = 0xFFFFu;  // the tag of the small kinds (a prime's index is at most 65534)
constexpr uint32_t kSampleTernaryK = 0, kSampleCbdK = 1;

struct sample_key {
    uint32_t w[8];      // the 32 key bytes as little-endian words: state words 4 .. 11
};

AGX_SAMPLE_HD uint32_t sample_rotl(uint32_t x, int k) {
#if defined(__has_builtin)
#if __has_builtin(__builtin_rotateleft32)
    return __builtin_rotateleft32(x, (uint32_t)k);      // one v_alignbit_b32 on the device
#else
    return (x << k) | (x >> (32 - k));
#endif
#else
    return (x << k) | (x >> (32 - k));
#endif
}

AGX_SAMPLE_HD void sample_quarter_round(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    a += b, d ^= a, d = sample_rotl(d, 16);
    c += d, b ^= c, b = sample_rotl(b, 12);
    a += b, d ^= a, d = sample_rotl(d, 8);
    c += d, b ^= c, b = sample_rotl(b, 7);
}

AGX_SAMPLE_HD void sample_block(const sample_key& key, uint32_t w12, uint32_t w13, uint32_t w14, uint32_t w15, uint32_t o[16]) {
    const uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.w[0], key.w[1], key.w[2], key.w[3],
                            key.w[4],    key.w[5],    key.w[6],    key.w[7],    w12,      w13,      w14,      w15};
    uint32_t x0 = s[0], x1 = s[1], x2 = s[2], x3 = s[3], x4 = s[4], x5 = s[5], x6 = s[6], x7 = s[7];
    uint32_t x8 = s[8], x9 = s[9], x10 = s[10], x11 = s[11], x12 = s[12], x13 = s[13], x14 = s[14], x15 = s[15];
    for (int round = 0; round < 10; ++round) {
        sample_quarter_round(x0, x4, x8, x12), sample_quarter_round(x1, x5, x9, x13), sample_quarter_round(x2, x6, x10, x14), sample_quarter_round(x3, x7, x11, x15);
        sample_quarter_round(x0, x5, x10, x15), sample_quarter_round(x1, x6, x11, x12), sample_quarter_round(x2, x7, x8, x13), sample_quarter_round(x3, x4, x9, x14);
    }
    o[0] = x0 + s[0], o[1] = x1 + s[1], o[2] = x2 + s[2], o[3] = x3 + s[3], o[4] = x4 + s[4], o[5] = x5 + s[5], o[6] = x6 + s[6], o[7] = x7 + s[7];
    o[8] = x8 + s[8], o[9] = x9 + s[9], o[10] = x10 + s[10], o[11] = x11 + s[11], o[12] = x12 + s[12], o[13] = x13 + s[13], o[14] = x14 + s[14], o[15] = x15 + s[15];
}

AGX_SAMPLE_HD uint64_t sample_candidate(const uint32_t o[16], int i) { return (uint64_t)o[2 * i] | ((uint64_t)o[2 * i + 1] << 32); }

AGX_SAMPLE_HD uint32_t sample_w12(uint32_t tag, uint32_t cell, uint32_t k) { return tag << 16 | cell << 4 | k; }
AGX_SAMPLE_HD uint64_t sample_mask(uint64_t q) { return ~(uint64_t)0 >> __builtin_clzll(q); }      // 2^bitlen(q) - 1, q >= 1

// out[0 .. 7]: the W <= 8 words of a uniform cell under q, the rest 0.  block_of(k, o) fills o[0 .. 15] with block k of the cell.  Every index of out is a
// constant once the two inner loops are unrolled (a word goes to its place through selects), so the eight words live in registers on the device; a block
// whose eight candidates all pass while no word is placed yet -- every block 0 but about W (1 - q / 2^bitlen(q)) of them -- is taken as it stands.
template <class BlockOf>
AGX_SAMPLE_HD void sample_uniform_cell(BlockOf&& block_of, uint64_t q, uint64_t mask, uint32_t W, uint64_t out[8]) {
    AGX_SAMPLE_UNROLL
    for (int s = 0; s < 8; ++s) out[s] = 0;
    uint32_t r = 0;
    for (uint32_t k = 0; k < kSampleMaxBlocks && r < W; ++k) {
        uint32_t o[16];
        block_of(k, o);
        uint64_t v[8];
        bool all = true;
        AGX_SAMPLE_UNROLL
        for (int i = 0; i < 8; ++i) v[i] = sample_candidate(o, i) & mask, all = all && v[i] < q;
        if (all && r == 0 && W == 8) {
            AGX_SAMPLE_UNROLL
            for (int i = 0; i < 8; ++i) out[i] = v[i];
            r = 8;
        } else {
            AGX_SAMPLE_UNROLL
            for (int i = 0; i < 8; ++i) {
                const bool take = v[i] < q && r < W;
                AGX_SAMPLE_UNROLL
                for (int s = 0; s < 8; ++s) out[s] = take && r == (uint32_t)s ? v[i] : out[s];
                r += take ? 1u : 0u;
            }
        }
    }
}

AGX_SAMPLE_HD int32_t sample_ternary(uint64_t w) {
    const uint64_t m = ~w, marks = ((m | (m >> 1)) & 0x5555555555555555ull) | ((uint64_t)1 << 62);
    const uint32_t f = (uint32_t)(w >> __builtin_ctzll(marks)) & 3u;
    return (int32_t)(f & 1u) - (int32_t)(f >> 1);
}

AGX_SAMPLE_HD uint32_t sample_eta_mask(uint32_t eta) { return eta >= 32 ? 0xffffffffu : (1u << eta) - 1u; }      // 1 <= eta <= 32

AGX_SAMPLE_HD int32_t sample_cbd(uint64_t w, uint32_t eta_mask) {
    return (int32_t)__builtin_popcount((uint32_t)w & eta_mask) - (int32_t)__builtin_popcount((uint32_t)(w >> 32) & eta_mask);
}

AGX_SAMPLE_HD uint64_t sample_residue(int32_t v, uint64_t q) {
    uint64_t mag = (uint64_t)(v < 0 ? -v : v);
    while (mag >= q) mag -= q;      // q <= 32 only
    return v < 0 && mag ? q - mag : mag;
}

}  // namespace agx
