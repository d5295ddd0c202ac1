// inner_selftest.cpp -- the host-compilable parts of agx_ntt_inner_product and agx_ntt_keyswitch_* against brute force in unsigned __int128.
// Stand-alone: built from this file, tests/selftest.hpp and the two headers alone by tests/test_selftests.py with -fsanitize=address,undefined; no HIP, no plan.
//   (a) csrc/inner_reduce.hpp, the very text the kernel compiles: acc_mul_add / acc_reduce against (sum of products) % q for 1, 2, 15 and 16 terms,
//       all operands q - 1 and random ones; acc_reduce on random and extreme 128-bit values; moduli of the 2-, 17-, 30-, 31-, 60-, 61- and 62-bit
//       classes (2^62 - 57 and its neighbours included).  The largest multiple of q left before the conditional subtracts is reported (must be <= 3).
//   (b) csrc/keyswitch_layout.hpp: the shape rules, digit ranges for q_count not a multiple of alpha, a scratch partition whose parts are disjoint,
//       ordered and sum to the reported total, counts past 2^60 words reported and not wrapped, the launch count.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../agilex-ntt_amd/csrc/inner_reduce.hpp"
#include "../agilex-ntt_amd/csrc/keyswitch_layout.hpp"
#include "selftest.hpp"

static uint64_t g_worst_multiple = 0;

struct modulus {
    uint64_t q, mu_hi, mu_lo;
    explicit modulus(uint64_t q_) : q(q_) {
        const u128 mu = ~(u128)0 / q_;      // floor(2^128 / q) for odd q > 1, as plan creation computes it
        mu_hi = (uint64_t)(mu >> 64), mu_lo = (uint64_t)mu;
    }
};

static void check_value(const modulus& m, u128 x) {
    agx::acc128 s;
    s.lo = (uint64_t)x, s.hi = (uint64_t)(x >> 64);
    const uint64_t want = (uint64_t)(x % m.q);
    const uint64_t lazy = agx::acc_reduce_lazy(s, m.q, m.mu_hi, m.mu_lo);
    CHECK(lazy % m.q == want && lazy / m.q <= 3, "q=%llu: lazy remainder %llu, want %llu", (unsigned long long)m.q, (unsigned long long)lazy, (unsigned long long)want);
    if (lazy / m.q > g_worst_multiple) g_worst_multiple = lazy / m.q;
    const uint64_t got = agx::acc_reduce(s, m.q, m.mu_hi, m.mu_lo);
    CHECK(got == want, "q=%llu: reduced %llu, want %llu", (unsigned long long)m.q, (unsigned long long)got, (unsigned long long)want);
}

static void check_sum(const modulus& m, int terms, bool extreme) {
    agx::acc128 s;
    u128 want = 0;
    for (int t = 0; t < terms; ++t) {
        const uint64_t a = extreme ? m.q - 1 : next64() % m.q, b = extreme ? m.q - 1 : next64() % m.q;
        agx::acc_mul_add(s, a, b);
        want += (u128)a * b;      // sixteen products below 2^124 each: no wrap
    }
    CHECK(s.lo == (uint64_t)want && s.hi == (uint64_t)(want >> 64), "q=%llu terms=%d: the 128-bit sum differs", (unsigned long long)m.q, terms);
    check_value(m, want);
}

static void test_reduce() {
    const uint64_t moduli[] = {3, 65537, 114689, (1ull << 30) - 35, 1073479681ull, (1ull << 31) + 11, (1ull << 31) - 1, (1ull << 60) - 93, 1152921504606830593ull,
                               (1ull << 61) + 1, (1ull << 61) - 1, (1ull << 62) - 57, (1ull << 62) - 1, (1ull << 62) - 87, 4611686018427322369ull};
    for (uint64_t q : moduli) {
        const modulus m(q);
        for (int terms : {1, 2, 15, 16}) {
            check_sum(m, terms, true);
            for (int k = 0; k < 2000; ++k) check_sum(m, terms, false);
        }
        const u128 top = ~(u128)0;
        for (u128 x : {(u128)0, (u128)1, (u128)q - 1, (u128)q, (u128)q + 1, top, top - 1, top - q, (u128)1 << 64, ((u128)1 << 64) - 1, (u128)q << 64, (u128)q * q,
                       (u128)16 * (q - 1) * (q - 1)})
            check_value(m, x);
        for (int k = 0; k < 20000; ++k) check_value(m, ((u128)next64() << 64) | next64());
        for (int k = 0; k < 2000; ++k) check_value(m, top - next64());      // the top of the range, where x / 2^128 is nearly 1
    }
    std::printf("acc_reduce: worst multiple of q before the subtracts: %llu\n", (unsigned long long)g_worst_multiple);
}

static void test_layout() {
    using agx::keyswitch_shape;
    // shape rules on a plan of six primes
    CHECK(agx::keyswitch_shape_ok({4, 4, 2, 2}, 6), "top level");
    CHECK(agx::keyswitch_shape_ok({3, 4, 2, 2}, 6), "one level down");
    CHECK(agx::keyswitch_shape_ok({4, 5, 1, 1}, 6), "four digits");
    CHECK(!agx::keyswitch_shape_ok({0, 4, 2, 2}, 6) && !agx::keyswitch_shape_ok({4, 4, 0, 2}, 6) && !agx::keyswitch_shape_ok({4, 4, 2, 0}, 6), "zero counts");
    CHECK(!agx::keyswitch_shape_ok({4, 3, 2, 2}, 6), "special primes inside Q");
    CHECK(!agx::keyswitch_shape_ok({4, 5, 2, 2}, 6) && !agx::keyswitch_shape_ok({4, 6, 1, 2}, 6) && !agx::keyswitch_shape_ok({4, 7, 1, 2}, 6), "a range past P");
    CHECK(!agx::keyswitch_shape_ok({4, 0xffffffffu, 2, 2}, 6) && !agx::keyswitch_shape_ok({4, 4, 0xffffffffu, 2}, 6), "ranges that would wrap");
    CHECK(!agx::keyswitch_shape_ok({20, 20, 2, 17}, 40) && !agx::keyswitch_shape_ok({20, 20, 17, 2}, 40), "more than 16 sources");
    CHECK(agx::keyswitch_shape_ok({16, 16, 2, 1}, 40) && !agx::keyswitch_shape_ok({17, 17, 2, 1}, 40), "sixteen digits, seventeen");
    CHECK(agx::keyswitch_shape_ok({256, 256, 16, 16}, 300) && !agx::keyswitch_shape_ok({257, 257, 16, 16}, 300), "sixteen digits of sixteen, one more prime");
    // digit ranges: they tile [0, q_count) in order, all of alpha primes but a short last one
    for (uint32_t q_count = 1; q_count <= 40; ++q_count)
        for (uint32_t alpha = 1; alpha <= 16; ++alpha) {
            const keyswitch_shape k{q_count, q_count, 1, alpha};
            CHECK(k.digits() == (q_count + alpha - 1) / alpha, "digits");
            uint32_t next = 0;
            for (uint32_t d = 0; d < k.digits(); ++d) {
                uint32_t first = 99, count = 99;
                agx::keyswitch_digit(k, d, &first, &count);
                CHECK(first == next && count >= 1 && count <= alpha && (count == alpha || d + 1 == k.digits()), "digit %u of q_count=%u alpha=%u", d, q_count, alpha);
                next = first + count;
            }
            CHECK(next == q_count, "the digits do not tile Q");
        }
    {
        const keyswitch_shape k{3, 4, 2, 2};
        uint32_t first, count;
        agx::keyswitch_digit(k, 1, &first, &count);
        CHECK(k.digits() == 2 && first == 2 && count == 1 && k.active() == 5 && k.apart(), "(3, 4, 2, 2): a short last digit");
    }
    // the scratch: three parts in order, disjoint, summing to the total
    for (const keyswitch_shape& k : {keyswitch_shape{4, 4, 2, 2}, keyswitch_shape{3, 4, 2, 2}, keyswitch_shape{4, 5, 1, 1}, keyswitch_shape{4, 4, 2, 4}, keyswitch_shape{7, 9, 3, 3}})
        for (uint32_t n : {2u, 64u, 4096u, 32768u})
            for (uint64_t batch : {(uint64_t)0, (uint64_t)1, (uint64_t)5, (uint64_t)4096}) {
                agx::keyswitch_scratch p;
                CHECK(agx::keyswitch_scratch_partition(k, n, batch, &p), "a small partition refused");
                const uint64_t slab = batch * n, coeff = k.q_count * slab, ext = (uint64_t)k.digits() * k.active() * slab, acc = 2ull * k.active() * slab;
                CHECK(p.coeff == 0 && p.ext == p.coeff + coeff && p.acc == p.ext + ext && p.total == p.acc + acc, "parts overlap or leave a gap");
                CHECK(p.total == coeff + ext + acc, "the parts do not sum to the total");
            }
    // counts past 2^60 words are reported, not wrapped
    {
        agx::keyswitch_scratch p;
        p.total = 77;
        const keyswitch_shape k{4, 4, 2, 2};
        CHECK(!agx::keyswitch_scratch_partition(k, 32768, (uint64_t)1 << 45, &p) && p.total == 77, "2^60 words per slab");
        CHECK(!agx::keyswitch_scratch_partition(k, 4096, ~(uint64_t)0, &p) && p.total == 77, "the largest batch");
        CHECK(!agx::keyswitch_scratch_partition(k, 2, (uint64_t)1 << 63, &p), "batch n = 2^64 would wrap 64 bits to zero");
        CHECK(!agx::keyswitch_scratch_partition(k, 32768, (uint64_t)1 << 49, &p), "batch n = 2^64");
        // the total passes 2^60 although every part is below it: (4 + 2 6 + 2 6) = 28 slabs of 2^56 words
        CHECK(!agx::keyswitch_scratch_partition(k, 32768, (uint64_t)1 << 41, &p), "a total past 2^60");
        CHECK(agx::keyswitch_scratch_partition(k, 32768, (uint64_t)1 << 40, &p) && p.total == 28ull << 55, "28 slabs of 2^55 words");
        const keyswitch_shape wide{256, 256, 16, 16};      // 256 + 16 272 + 2 272 = 5152 slabs
        CHECK(agx::keyswitch_scratch_partition(wide, 2, (uint64_t)1 << 46, &p) && p.total == 5152ull << 47, "5152 slabs of 2^47 words");
        CHECK(!agx::keyswitch_scratch_partition(wide, 2, (uint64_t)1 << 47, &p), "5152 slabs of 2^48 words");
    }
    // launches
    {
        const int one[] = {1, 1}, pairs[] = {2, 2, 2, 2};
        CHECK(agx::keyswitch_launches(1, one, 2, 2) == 1 + 2 + 1 + 4, "two digits, fused routes");
        CHECK(agx::keyswitch_launches(2, pairs, 4, 7) == 2 + 8 + 1 + 14, "two digits apart, radix-2 at n = 32768");
        CHECK(agx::keyswitch_launches(1, nullptr, 0, 4) == 1 + 1 + 8, "no ModUp call");
    }
}

int main() {
    test_reduce();
    selftest_section("inner_reduce");
    test_layout();
    return selftest_report("keyswitch_layout");
}
