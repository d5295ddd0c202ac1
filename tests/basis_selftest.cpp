// basis_selftest.cpp -- agx::basis_constants (csrc/host_math.cpp), the host side of agx_ntt_basis_extend, against brute force in unsigned __int128.
// Stand-alone: built from this file, tests/selftest.hpp and host_math.cpp by tests/test_selftests.py with -fsanitize=address,undefined; no HIP, no plan.
//   * every constant against its definition, the products taken in another order than the builder takes them: D_i^-1 D_i = 1 (mod q_i),
//     mat[j][i] = D_i mod q_j, every quotient = floor(w 2^64 / q);
//   * where S D fits 128 bits, the conversion itself: for X in [0, D) with residues x_i, V = sum_i y_i D_i as an exact integer is X + u D with
//     0 <= u < S, and sum_i y_i mat[j][i] mod q_j is V mod q_j -- X = 0, 1, D - 1, the neighbours of the multiples of D / 2 and random X;
//   * S = 1, 2, 16 (and what lies between while it fits), 17-, 30-, 60- and 62-bit-class primes and mixtures of them;
//   * a target that is itself a source: its row is zero but for that source, whose entry undoes D_k^-1; equal source moduli: refused.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../agilex-ntt_amd/csrc/host_math.hpp"
#include "selftest.hpp"

// D_i mod m, from the last factor to the first (the builder goes first to last)
static uint64_t d_mod_brute(const std::vector<uint64_t>& src, size_t i, uint64_t m) {
    u128 r = 1 % m;
    for (size_t k = src.size(); k-- > 0;)
        if (k != i) r = r * (u128)(src[k] % m) % m;
    return (uint64_t)r;
}

struct built {
    bool ok;
    std::vector<uint64_t> dinv, dinv_p, mat, mat_p;
};
static built build(const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst) {
    const size_t S = src.size(), T = dst.size();
    // exact sizes: the sanitizer sees a write past [S] or [T][S]
    built b{false, std::vector<uint64_t>(S), std::vector<uint64_t>(S), std::vector<uint64_t>(T * S), std::vector<uint64_t>(T * S)};
    b.ok = agx::basis_constants(src.data(), (uint32_t)S, dst.data(), (uint32_t)T, b.dinv.data(), b.dinv_p.data(), b.mat.data(), b.mat_p.data());
    return b;
}

static void check_constants(const char* what, const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst) {
    const size_t S = src.size(), T = dst.size();
    const built b = build(src, dst);
    CHECK(b.ok, "%s: refused", what);
    if (!b.ok) return;
    for (size_t i = 0; i < S; ++i) {
        const uint64_t q = src[i];
        CHECK(b.dinv[i] < q, "%s: dinv[%zu] not reduced", what, i);
        CHECK((uint64_t)((u128)b.dinv[i] * d_mod_brute(src, i, q) % q) == 1 % q, "%s: dinv[%zu] is not the inverse of D_i", what, i);
        CHECK(b.dinv_p[i] == (uint64_t)(((u128)b.dinv[i] << 64) / q), "%s: quotient of dinv[%zu]", what, i);
    }
    for (size_t j = 0; j < T; ++j)
        for (size_t i = 0; i < S; ++i) {
            const uint64_t q = dst[j], c = b.mat[j * S + i];
            CHECK(c == d_mod_brute(src, i, q), "%s: mat[%zu][%zu]", what, j, i);
            CHECK(b.mat_p[j * S + i] == (uint64_t)(((u128)c << 64) / q), "%s: quotient of mat[%zu][%zu]", what, j, i);
            // a target that is source k: D_i holds the factor q_k for i != k, and D_k times its inverse is 1
            for (size_t k = 0; k < S; ++k)
                if (src[k] == q) {
                    if (i != k) CHECK(c == 0, "%s: target %zu is source %zu, mat[%zu][%zu] != 0", what, j, k, j, i);
                    else CHECK((uint64_t)((u128)c * b.dinv[k] % q) == 1 % q, "%s: target %zu is source %zu: the residue is not handed through", what, j, k);
                }
        }
}

// the conversion in exact integers; needs S D < 2^128
static void check_conversion(const char* what, const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, int random_values) {
    const size_t S = src.size(), T = dst.size();
    const built b = build(src, dst);
    CHECK(b.ok, "%s: refused", what);
    if (!b.ok) return;
    u128 D = 1;
    std::vector<u128> Di(S, 1);
    for (size_t i = 0; i < S; ++i) {
        D *= src[i];
        for (size_t k = 0; k < S; ++k)
            if (k != i) Di[i] *= src[k];
    }
    std::vector<u128> xs = {0, 1, D - 1, D / 2, D / 2 - 1, D / 2 + 1, D - 2};
    for (int k = 0; k < random_values; ++k) xs.push_back(next128() % D);
    // V = X + u D: X = 0, 1, D - 1 put V on a multiple of D or next to one
    for (const u128 X : xs) {
        u128 V = 0;
        std::vector<uint64_t> y(S);
        for (size_t i = 0; i < S; ++i) {
            y[i] = (uint64_t)((u128)(uint64_t)(X % src[i]) * b.dinv[i] % src[i]);
            V += (u128)y[i] * Di[i];
        }
        CHECK(V % D == X % D, "%s: V is not congruent to X modulo D", what);
        CHECK(V / D < S, "%s: u = V / D is not below S", what);
        for (size_t j = 0; j < T; ++j) {
            u128 acc = 0;      // at most 16 2^62 2^62: needs every bit of 128 at S = 16; here S D < 2^128 keeps it far below
            for (size_t i = 0; i < S; ++i) acc += (u128)y[i] * b.mat[j * S + i];
            CHECK((uint64_t)(acc % dst[j]) == (uint64_t)(V % dst[j]), "%s: target %zu", what, j);
            for (size_t k = 0; k < S; ++k)
                if (src[k] == dst[j]) CHECK((uint64_t)(acc % dst[j]) == (uint64_t)(X % dst[j]), "%s: target %zu is source %zu but not its residue", what, j, k);
        }
    }
}

static std::vector<uint64_t> primes(uint32_t bits, uint32_t n, uint32_t count) {
    std::vector<uint64_t> p = agx::find_ntt_primes(bits, n, count);
    CHECK(p.size() == count, "find_ntt_primes(%u, %u, %u) found %zu", bits, n, count, p.size());
    return p;
}
static std::vector<uint64_t> slice(const std::vector<uint64_t>& v, size_t lo, size_t hi) { return std::vector<uint64_t>(v.begin() + lo, v.begin() + hi); }

int main() {
    const struct {
        uint32_t bits, n;
    } classes[] = {{17, 8}, {30, 64}, {60, 4096}, {62, 1024}};
    for (const auto& c : classes) {
        const std::vector<uint64_t> p = primes(c.bits, c.n, 17);
        if (p.size() != 17) continue;
        char what[96];
        for (size_t S : {(size_t)1, (size_t)2, (size_t)3, (size_t)5, (size_t)16}) {
            std::snprintf(what, sizeof what, "%u-bit, S = %zu -> all 17", c.bits, S);
            check_constants(what, slice(p, 0, S), p);                      // ModUp: the targets contain the sources
            std::snprintf(what, sizeof what, "%u-bit, S = %zu -> the others", c.bits, S);
            check_constants(what, slice(p, 17 - S, 17), slice(p, 0, 17 - S));      // ModDown: disjoint
            std::snprintf(what, sizeof what, "%u-bit, S = %zu -> itself", c.bits, S);
            check_constants(what, slice(p, 1, 1 + S), slice(p, 1, 1 + S));
        }
        // the conversion itself while S D fits 128 bits: S * bits + log2(S) <= 128, log2(S) <= 4
        for (size_t S = 1; S <= 16 && S * c.bits + 4 <= 128; ++S) {
            std::snprintf(what, sizeof what, "conversion, %u-bit, S = %zu", c.bits, S);
            check_conversion(what, slice(p, 0, S), p, 200);
        }
        // equal source moduli: D_i is not invertible
        std::vector<uint64_t> twice = {p[0], p[1], p[0]};
        CHECK(!build(twice, p).ok, "%u-bit: equal source moduli accepted", c.bits);
        CHECK(!build({p[3], p[3]}, {p[0]}).ok, "%u-bit: a source given twice accepted", c.bits);
        std::vector<uint64_t> sixteen_and_one = slice(p, 0, 16);
        sixteen_and_one[15] = p[0];
        CHECK(!build(sixteen_and_one, p).ok, "%u-bit: S = 16 with the first modulus repeated accepted", c.bits);
    }
    // mixed widths: a 30-bit source lifted under 62-bit targets and the other way round, and the widths of one RNS chain together
    const std::vector<uint64_t> mixed = {primes(60, 1024, 1)[0], primes(30, 1024, 1)[0], primes(61, 1024, 1)[0], primes(30, 1024, 2)[1], primes(62, 1024, 1)[0],
                                         primes(17, 8, 1)[0]};
    check_constants("mixed widths, all -> all", mixed, mixed);
    check_conversion("mixed widths, [30, 61] -> all", {mixed[1], mixed[2]}, mixed, 500);
    check_conversion("mixed widths, [62, 17, 30] -> all", {mixed[4], mixed[5], mixed[3]}, mixed, 500);
    check_conversion("mixed widths, [17] -> all", {mixed[5]}, mixed, 500);
    return selftest_report("basis_constants");
}
