// weighted_selftest.cpp -- csrc/weighted_arith.hpp, the per-word finish of agx_ntt_keyswitch_accumulate_decomposed and agx_ntt_mul_add_galois and the very
// text the kernels compile, against unsigned __int128.  Stand-alone: built from this file, tests/selftest.hpp, weighted_arith.hpp, ring_arith.hpp and
// inner_reduce.hpp alone by tests/test_selftests.py with -fsanitize=address,undefined; no HIP, no plan.
//   Moduli: the arguments (tests/test_selftests.py passes the class edges of tests/modulus_cases.py: the primes next to 2^31, 2^60 and 2^62, those
//   next to 2^60 - 2^28, the smallest admitted primes), and always the built-in list below.  The finish asks for an odd q < 2^62 only.
//   Operands: the weight and the old word at 0, 1, q - 1, q, 2q, 4q - 1 (and 2^64 - 1 where 4q exceeds it, which no admitted modulus reaches: 4q < 2^64),
//   t at 0, 1, q - 1; random words over the whole ranges; with the old word present and absent, with the weight present and absent.
//   The whole word: sixteen products of lazy operands summed in 128 bits, reduced, then finished, against the same in big integers.
//   The range argument: w' t + old' stays below 2^124 + 2^62 at the largest operands.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../agilex-ntt_amd/csrc/weighted_arith.hpp"
#include "selftest.hpp"

struct modulus {
    uint64_t q, q2, mu_hi, mu_lo;
    explicit modulus(uint64_t q_) : q(q_), q2(q_ << 1) {
        const u128 mu = ~(u128)0 / q_;      // floor(2^128 / q) for odd q > 1, as plan creation computes it
        mu_hi = (uint64_t)(mu >> 64), mu_lo = (uint64_t)mu;
    }
};

static std::vector<uint64_t> edges(uint64_t q) {
    std::vector<uint64_t> e = {0, 1, q - 1, q, 2 * q, 4 * q - 1};
    if ((u128)4 * q > ~0ull) e.push_back(~0ull);
    return e;
}

static uint64_t lazy(uint64_t q) { return (uint64_t)(next128() % ((u128)4 * q)); }      // uniform over [0, 4q)
static uint64_t reduced(uint64_t q) { return (uint64_t)(next128() % q); }

static void check_word(const modulus& m, uint64_t w, uint64_t t, uint64_t old) {
    const uint64_t q = m.q;
    const u128 W = w % q, T = t, O = old % q;
    CHECK(W * T + O < ((u128)1 << 124) + ((u128)1 << 62), "q=%llu: the 128-bit sum leaves its range", (unsigned long long)q);
    const uint64_t both = agx::weighted_finish(t, true, w, true, old, q, m.q2, m.mu_hi, m.mu_lo);
    const uint64_t no_old = agx::weighted_finish(t, true, w, false, old, q, m.q2, m.mu_hi, m.mu_lo);      // old is not looked at
    const uint64_t no_w = agx::weighted_finish(t, false, w, true, old, q, m.q2, m.mu_hi, m.mu_lo);        // w is not looked at
    const uint64_t neither = agx::weighted_finish(t, false, w, false, old, q, m.q2, m.mu_hi, m.mu_lo);
    CHECK(both == (uint64_t)((W * T + O) % q), "q=%llu: %llu + %llu x %llu gave %llu", (unsigned long long)q, (unsigned long long)old, (unsigned long long)w,
          (unsigned long long)t, (unsigned long long)both);
    CHECK(no_old == (uint64_t)(W * T % q), "q=%llu: %llu x %llu gave %llu", (unsigned long long)q, (unsigned long long)w, (unsigned long long)t, (unsigned long long)no_old);
    CHECK(no_w == (uint64_t)((T + O) % q), "q=%llu: %llu + %llu gave %llu", (unsigned long long)q, (unsigned long long)old, (unsigned long long)t, (unsigned long long)no_w);
    CHECK(neither == t, "q=%llu: %llu alone gave %llu", (unsigned long long)q, (unsigned long long)t, (unsigned long long)neither);
    CHECK(agx::weighted_mul_add(w, t, old, q, m.q2, m.mu_hi, m.mu_lo) == both, "q=%llu: weighted_mul_add differs from weighted_finish", (unsigned long long)q);
}

// the word as the kernel forms it: `terms` products of lazy operands in one acc128, acc_reduce, then the finish
static void check_chain(const modulus& m, int terms, bool largest) {
    const uint64_t q = m.q;
    agx::acc128 s;
    u128 sum = 0;
    for (int t = 0; t < terms; ++t) {
        const uint64_t a = largest ? q - 1 + (uint64_t)(t & 3) * q : lazy(q), b = largest ? 4 * q - 1 : lazy(q);
        agx::acc_mul_add(s, agx::ring_reduce(a, q, m.q2), agx::ring_reduce(b, q, m.q2));
        sum = (sum + (u128)(a % q) * (b % q) % q) % q;
    }
    const uint64_t t = agx::acc_reduce(s, q, m.mu_hi, m.mu_lo);
    CHECK(t == (uint64_t)sum, "q=%llu: the sum of %d terms", (unsigned long long)q, terms);
    const uint64_t w = largest ? 4 * q - 1 : lazy(q), old = largest ? 4 * q - 1 : lazy(q);
    const uint64_t got = agx::weighted_finish(t, true, w, true, old, q, m.q2, m.mu_hi, m.mu_lo);
    CHECK(got == (uint64_t)(((u128)(w % q) * sum + old % q) % q) && got < q, "q=%llu: the finished word of %d terms", (unsigned long long)q, terms);
}

int main(int argc, char** argv) {
    std::vector<uint64_t> moduli = {3, 65537, 114689, (1ull << 30) - 35, 1073479681ull, (1ull << 31) + 11, (1ull << 31) - 1, (1ull << 60) - 93, 1152921504606830593ull,
                                    (1ull << 61) + 1, (1ull << 61) - 1, (1ull << 62) - 57, (1ull << 62) - 1, (1ull << 62) - 87, 4611686018427322369ull};
    for (int i = 1; i < argc; ++i) {
        const uint64_t q = std::strtoull(argv[i], nullptr, 10);
        if (q < 3 || !(q & 1) || q >= (1ull << 62)) {
            std::printf("not an odd modulus in [3, 2^62): %s\n", argv[i]);
            return 2;
        }
        moduli.push_back(q);
    }
    for (uint64_t q : moduli) {
        const modulus m(q);
        const std::vector<uint64_t> e = edges(q);
        const uint64_t ts[] = {0, 1 % q, q - 1, q / 2, reduced(q)};
        for (uint64_t w : e)
            for (uint64_t old : e)
                for (uint64_t t : ts) check_word(m, w, t, old);
        for (uint64_t x : e)
            for (int k = 0; k < 40; ++k) check_word(m, x, reduced(q), lazy(q)), check_word(m, lazy(q), reduced(q), x);
        for (int k = 0; k < 4000; ++k) check_word(m, lazy(q), reduced(q), lazy(q));
        for (int terms : {1, 2, 3, 4, 15, 16}) {
            check_chain(m, terms, true);
            for (int k = 0; k < 100; ++k) check_chain(m, terms, false);
        }
    }
    std::printf("moduli: %zu\n", moduli.size());
    return selftest_report("weighted_arith");
}
