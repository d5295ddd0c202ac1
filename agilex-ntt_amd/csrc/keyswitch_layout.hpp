// keyswitch_layout.hpp -- the integer arithmetic of agx_ntt_keyswitch_*: shape rules, digit ranges, the partition of the scratch and the launch
// count.  No HIP, no plan: tests/inner_selftest.cpp checks it on a CPU.  Everything is counted in 8-byte words.
//   Q = plan primes [0, q_count), the special primes = [p_first, p_first + p_count) with p_first >= q_count, A = q_count + p_count active primes
//   in that order; digit d = primes [d alpha, min((d + 1) alpha, q_count)), digits = ceil(q_count / alpha).
#pragma once
#include <cstdint>

namespace agx {

constexpr uint32_t kKeyswitchMaxDigits = 16;      // AGX_KEYSWITCH_MAX_DIGITS = AGX_INNER_MAX_TERMS: the digits are the terms of one inner product
constexpr uint32_t kKeyswitchMaxSources = 16;     // AGX_BASIS_MAX_SRC: a digit and the special primes are each the sources of a basis

struct keyswitch_shape {
    uint32_t q_count = 0, p_first = 0, p_count = 0, alpha = 0;
    uint32_t active() const { return q_count + p_count; }
    uint32_t digits() const { return q_count / alpha + (q_count % alpha ? 1u : 0u); }      // no sum that could wrap
    bool apart() const { return p_first != q_count; }      // a level below the top: Q and the special primes are two ranges of the plan
};

// agx_ntt_keyswitch_create's rules on the numbers alone, for a plan of num_primes primes
inline bool keyswitch_shape_ok(const keyswitch_shape& k, uint32_t num_primes) {
    if (k.q_count == 0 || k.p_count == 0 || k.alpha == 0) return false;
    if (k.alpha > kKeyswitchMaxSources || k.p_count > kKeyswitchMaxSources) return false;
    if (k.p_first < k.q_count || k.p_first > num_primes || k.p_count > num_primes - k.p_first) return false;      // q_count <= p_first <= P follows
    return k.digits() <= kKeyswitchMaxDigits;
}

// digit d < digits(): its first prime and how many it has (the last digit may be short)
inline void keyswitch_digit(const keyswitch_shape& k, uint32_t d, uint32_t* first, uint32_t* count) {
    *first = d * k.alpha;
    *count = k.q_count - *first < k.alpha ? k.q_count - *first : k.alpha;
}

// The scratch of one apply call, three dense parts one behind the other:
//   coeff [q_count][batch][n]          INTT_j(chat_j), the sources of every digit's conversion
//   ext   [digits][A][batch][n]        NTT_j(e_{d,j}): the `a` operand of the inner product
//   acc   [2][A][batch][n]             the inner product's result; the special slabs of each half double as ModDown's scratch
struct keyswitch_scratch {
    uint64_t coeff = 0, ext = 0, acc = 0;      // word offsets of the parts
    uint64_t total = 0;
};

// false when batch n, any part or the total would pass 2^60 words (reported, never wrapped: 128-bit arithmetic; at most (1 + 16 32 + 2 32) 2^60 here)
inline bool keyswitch_scratch_partition(const keyswitch_shape& k, uint32_t n, uint64_t batch, keyswitch_scratch* out) {
    using u128 = unsigned __int128;
    const u128 limit = (u128)1 << 60;
    const u128 slab = (u128)batch * n;
    const u128 coeff = slab * k.q_count, ext = slab * k.active() * k.digits(), acc = slab * k.active() * 2;
    if (slab > limit || coeff > limit || ext > limit || acc > limit || coeff + ext + acc > limit) return false;
    out->coeff = 0;
    out->ext = (uint64_t)coeff;
    out->acc = (uint64_t)(coeff + ext);
    out->total = (uint64_t)(coeff + ext + acc);
    return true;
}

// The buffers of the two halves of an apply call (agx_ntt_keyswitch_decompose, agx_ntt_keyswitch_apply_decomposed), each one dense part of the above
// in a buffer of its own:
//   ext               [digits][A][batch][n]   what decompose writes and apply_decomposed reads: keyswitch_scratch's ext part
//   decompose_scratch [q_count][batch][n]     its coeff part
//   apply_scratch     [2][A][batch][n]        its acc part
struct keyswitch_hoisted {
    uint64_t ext = 0, decompose_scratch = 0, apply_scratch = 0;      // sizes in words
};

// false when batch n or any of the three would pass 2^60 words (128-bit arithmetic, as above).  The three are the sizes of keyswitch_scratch's parts;
// their sum is not limited here: no call takes the three in one buffer.
inline bool keyswitch_hoisted_partition(const keyswitch_shape& k, uint32_t n, uint64_t batch, keyswitch_hoisted* out) {
    using u128 = unsigned __int128;
    const u128 limit = (u128)1 << 60;
    const u128 slab = (u128)batch * n;
    const u128 coeff = slab * k.q_count, ext = slab * k.active() * k.digits(), acc = slab * k.active() * 2;
    if (slab > limit || coeff > limit || ext > limit || acc > limit) return false;
    out->ext = (uint64_t)ext;
    out->decompose_scratch = (uint64_t)coeff;
    out->apply_scratch = (uint64_t)acc;
    return true;
}

// kernel launches of the first half of an apply call: the inverse of Q and every ModUp call (extend[0 .. extend_calls): one per digit, two where the
// special primes lie apart)
inline int keyswitch_launches_decompose(int inverse, const int* extend, uint32_t extend_calls) {
    int total = inverse;
    for (uint32_t i = 0; i < extend_calls; ++i) total += extend[i];
    return total;
}

// of the second half: one inner product, two ModDown calls
inline int keyswitch_launches_apply_decomposed(int mod_down) { return 1 + 2 * mod_down; }

// of one apply call: both halves
inline int keyswitch_launches(int inverse, const int* extend, uint32_t extend_calls, int mod_down) {
    return keyswitch_launches_decompose(inverse, extend, extend_calls) + keyswitch_launches_apply_decomposed(mod_down);
}

}  // namespace agx
