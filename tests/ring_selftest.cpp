// ring_selftest.cpp -- csrc/ring_arith.hpp, the per-word arithmetic of agx_ntt_add / _sub / _negate / _add_galois / _tensor and the very text the kernels
// compile, against unsigned __int128.  Stand-alone: built from this file, tests/selftest.hpp, ring_arith.hpp and inner_reduce.hpp alone by
// tests/test_selftests.py with -fsanitize=address,undefined; no HIP, no plan.
//   add, sub, negate: every pair of the edge words 0, 1, q - 1, q, q + 1, 2q - 1, 2q, 2q + 1, 3q, 4q - 1 of the lazy input range, and random words over
//   the whole of [0, 4q); every result equals the big-integer one and lies below q; -0 = 0.
//   the tensor triple: a0 = a1 = b0 = b1 = q - 1 reduced and in every lazy representative, edge words, random words; squaring (a = b).
//   moduli of the 2-, 17-, 30-, 31-, 60-, 61- and 62-bit classes (2^62 - 57 and its neighbours included).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../agilex-ntt_amd/csrc/ring_arith.hpp"
#include "selftest.hpp"

struct modulus {
    uint64_t q, q2, mu_hi, mu_lo;
    explicit modulus(uint64_t q_) : q(q_), q2(q_ << 1) {
        const u128 mu = ~(u128)0 / q_;      // floor(2^128 / q) for odd q > 1, as plan creation computes it
        mu_hi = (uint64_t)(mu >> 64), mu_lo = (uint64_t)mu;
    }
};

static std::vector<uint64_t> edges(uint64_t q) { return {0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, 2 * q + 1, 3 * q, 4 * q - 1}; }

static uint64_t lazy(uint64_t q) { return (uint64_t)(next128() % ((u128)4 * q)); }      // uniform over [0, 4q)

static void check_linear(const modulus& m, uint64_t a, uint64_t b) {
    const uint64_t q = m.q, x = a % q, y = b % q;
    const uint64_t sum = agx::ring_add(a, b, q, m.q2), dif = agx::ring_sub(a, b, q, m.q2), neg = agx::ring_neg(a, q, m.q2);
    CHECK(sum == (uint64_t)(((u128)x + y) % q), "q=%llu: %llu + %llu gave %llu", (unsigned long long)q, (unsigned long long)a, (unsigned long long)b, (unsigned long long)sum);
    CHECK(dif == (uint64_t)(((u128)x + q - y) % q), "q=%llu: %llu - %llu gave %llu", (unsigned long long)q, (unsigned long long)a, (unsigned long long)b, (unsigned long long)dif);
    CHECK(neg == (q - x) % q && neg < q, "q=%llu: -%llu gave %llu", (unsigned long long)q, (unsigned long long)a, (unsigned long long)neg);
    CHECK(agx::ring_reduce(a, q, m.q2) == x, "q=%llu: %llu reduced wrongly", (unsigned long long)q, (unsigned long long)a);
}

static void check_tensor(const modulus& m, uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1) {
    const uint64_t q = m.q;
    uint64_t c0 = ~0ull, c1 = ~0ull, c2 = ~0ull;
    agx::ring_tensor(a0, a1, b0, b1, q, m.mu_hi, m.mu_lo, c0, c1, c2);
    const u128 x0 = a0 % q, x1 = a1 % q, y0 = b0 % q, y1 = b1 % q;      // products below 2^124, the cross sum below 2^125
    CHECK(c0 == (uint64_t)(x0 * y0 % q), "q=%llu: c0 of (%llu, %llu)", (unsigned long long)q, (unsigned long long)a0, (unsigned long long)b0);
    CHECK(c1 == (uint64_t)((x0 * y1 + x1 * y0) % q), "q=%llu: c1 of (%llu, %llu, %llu, %llu)", (unsigned long long)q, (unsigned long long)a0, (unsigned long long)a1,
          (unsigned long long)b0, (unsigned long long)b1);
    CHECK(c2 == (uint64_t)(x1 * y1 % q), "q=%llu: c2 of (%llu, %llu)", (unsigned long long)q, (unsigned long long)a1, (unsigned long long)b1);
}

int main() {
    const uint64_t moduli[] = {3, 65537, 114689, (1ull << 30) - 35, 1073479681ull, (1ull << 31) + 11, (1ull << 31) - 1, (1ull << 60) - 93, 1152921504606830593ull,
                               (1ull << 61) + 1, (1ull << 61) - 1, (1ull << 62) - 57, (1ull << 62) - 1, (1ull << 62) - 87, 4611686018427322369ull};
    for (uint64_t q : moduli) {
        const modulus m(q);
        const std::vector<uint64_t> e = edges(q);
        for (uint64_t a : e)
            for (uint64_t b : e) check_linear(m, a, b);
        for (uint64_t a : e)
            for (int k = 0; k < 50; ++k) check_linear(m, a, lazy(q)), check_linear(m, lazy(q), a);
        for (int k = 0; k < 8000; ++k) check_linear(m, lazy(q), lazy(q));
        // the largest operands: q - 1 in each of its four lazy representatives, independently per operand
        for (int r = 0; r < 256; ++r) check_tensor(m, q - 1 + (r & 3) * q, q - 1 + ((r >> 2) & 3) * q, q - 1 + ((r >> 4) & 3) * q, q - 1 + ((r >> 6) & 3) * q);
        for (uint64_t a0 : e)
            for (uint64_t a1 : e)
                for (uint64_t b0 : {e[0], e[2], e[3], e[9]})
                    for (uint64_t b1 : {e[1], e[2], e[6], e[9]}) check_tensor(m, a0, a1, b0, b1);
        for (int k = 0; k < 4000; ++k) check_tensor(m, lazy(q), lazy(q), lazy(q), lazy(q));
        for (int k = 0; k < 500; ++k) {      // squaring
            const uint64_t a0 = lazy(q), a1 = lazy(q);
            check_tensor(m, a0, a1, a0, a1);
        }
    }
    return selftest_report("ring_arith");
}
