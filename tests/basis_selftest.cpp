// basis_selftest.cpp -- agx::prepare_basis_image (csrc/host_math.cpp), the host side of agx_ntt_basis_extend, against brute force in unsigned __int128.
// Stand-alone: built from this file, tests/selftest.hpp and host_math.cpp by tests/test_selftests.py with -fsanitize=address,undefined; no HIP, no plan.
//   * every constant against its definition, the products taken in another order than the builder takes them: D_i^-1 D_i = 1 (mod q_i),
//     mat[j][i] = D_i mod q_j, every quotient = floor(w 2^64 / q);
//   * where S D fits 128 bits, the conversion itself: for X in [0, D) with residues x_i, V = sum_i y_i D_i as an exact integer is X + u D with
//     0 <= u < S, and sum_i y_i mat[j][i] mod q_j is V mod q_j -- X = 0, 1, D - 1, the neighbours of the multiples of D / 2 and random X;
//   * S = 1, 2, 16 (and what lies between while it fits), 17-, 30-, 60- and 62-bit-class primes and mixtures of them;
//   * a target that is itself a source: its row is zero but for that source, whose entry undoes D_k^-1; equal source moduli: refused;
//   * the golden record, its path the one argument: tests/golden/basis_constants.txt holds, for 22 requests (S = 1, 2, 3, 16, T = 1, 3, the 17-, 31-, 60-, 61-
//     and 62-bit classes mixed, t = 1, 65537, 2^64 - 59, no m, a 60-bit and a narrow m, targets that are sources, every refusal), every input and every word
//     the four builders wrote that prepare_basis_image replaced.  Every request is built again and every word of the file accounted for by one check: a
//     label is the expected one, an input is a number, an output is the image's word.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../agilex-ntt_amd/csrc/host_math.hpp"
#include "selftest.hpp"

typedef std::vector<uint64_t> vec;

// D_i mod m, from the last factor to the first (the builder goes first to last)
static uint64_t d_mod_brute(const vec& src, size_t i, uint64_t m) {
    u128 r = 1 % m;
    for (size_t k = src.size(); k-- > 0;)
        if (k != i) r = r * (u128)(src[k] % m) % m;
    return (uint64_t)r;
}

// the image of a plain request; the last-stage constants, which agx_ntt_basis_extend does not read, are ones
static bool build(agx::basis_image& img, const vec& src, const vec& dst) {
    const vec one(src.size(), 1);
    const bool ok = agx::prepare_basis_image(img, {src.data(), (uint32_t)src.size(), dst.data(), (uint32_t)dst.size(), one.data(), one.data()}) == agx::basis_fault::none;
    if (ok) CHECK(img.dinv.size() == src.size() && img.mat.size() == dst.size() * src.size(), "sizes [S], [T][S]");
    return ok;
}
static bool refused(const vec& src, const vec& dst) {
    agx::basis_image img;
    return !build(img, src, dst);
}

static void check_constants(const char* what, const vec& src, const vec& dst) {
    const size_t S = src.size(), T = dst.size();
    agx::basis_image b;
    const bool ok = build(b, src, dst);
    CHECK(ok, "%s: refused", what);
    if (!ok) return;
    for (size_t i = 0; i < S; ++i) {
        const uint64_t q = src[i];
        CHECK(b.dinv[i].w < q, "%s: dinv[%zu] not reduced", what, i);
        CHECK((uint64_t)((u128)b.dinv[i].w * d_mod_brute(src, i, q) % q) == 1 % q, "%s: dinv[%zu] is not the inverse of D_i", what, i);
        CHECK(b.dinv[i].p == (uint64_t)(((u128)b.dinv[i].w << 64) / q), "%s: quotient of dinv[%zu]", what, i);
    }
    for (size_t j = 0; j < T; ++j)
        for (size_t i = 0; i < S; ++i) {
            const uint64_t q = dst[j], c = b.mat[j * S + i].w;
            CHECK(c == d_mod_brute(src, i, q), "%s: mat[%zu][%zu]", what, j, i);
            CHECK(b.mat[j * S + i].p == (uint64_t)(((u128)c << 64) / q), "%s: quotient of mat[%zu][%zu]", what, j, i);
            // a target that is source k: D_i holds the factor q_k for i != k, and D_k times its inverse is 1
            for (size_t k = 0; k < S; ++k)
                if (src[k] == q) {
                    if (i != k) CHECK(c == 0, "%s: target %zu is source %zu, mat[%zu][%zu] != 0", what, j, k, j, i);
                    else CHECK((uint64_t)((u128)c * b.dinv[k].w % q) == 1 % q, "%s: target %zu is source %zu: the residue is not handed through", what, j, k);
                }
        }
}

// the conversion in exact integers; needs S D < 2^128
static void check_conversion(const char* what, const vec& src, const vec& dst, int random_values) {
    const size_t S = src.size(), T = dst.size();
    agx::basis_image b;
    const bool ok = build(b, src, dst);
    CHECK(ok, "%s: refused", what);
    if (!ok) return;
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
        vec y(S);
        for (size_t i = 0; i < S; ++i) {
            y[i] = (uint64_t)((u128)(uint64_t)(X % src[i]) * b.dinv[i].w % src[i]);
            V += (u128)y[i] * Di[i];
        }
        CHECK(V % D == X % D, "%s: V is not congruent to X modulo D", what);
        CHECK(V / D < S, "%s: u = V / D is not below S", what);
        for (size_t j = 0; j < T; ++j) {
            u128 acc = 0;      // at most 16 2^62 2^62: needs every bit of 128 at S = 16; here S D < 2^128 keeps it far below
            for (size_t i = 0; i < S; ++i) acc += (u128)y[i] * b.mat[j * S + i].w;
            CHECK((uint64_t)(acc % dst[j]) == (uint64_t)(V % dst[j]), "%s: target %zu", what, j);
            for (size_t k = 0; k < S; ++k)
                if (src[k] == dst[j]) CHECK((uint64_t)(acc % dst[j]) == (uint64_t)(X % dst[j]), "%s: target %zu is source %zu but not its residue", what, j, k);
        }
    }
}

// ---- the golden record: one CHECK per word of the file ----
static FILE* g_golden = nullptr;
static int g_record = -1;
static bool next_word(char* w) { return std::fscanf(g_golden, "%63s", w) == 1; }
static void expect_label(const char* label) {
    char w[64] = "";
    CHECK(next_word(w) && !std::strcmp(w, label), "record %d: read '%s' where '%s' belongs", g_record, w, label);
}
static bool number(uint64_t* v) {
    char w[64] = "", *end = w;
    const bool read = next_word(w);
    *v = std::strtoull(w, &end, 10);
    return read && end != w && *end == 0;
}
static uint64_t input(const char* what) {
    uint64_t v = 0;
    CHECK(number(&v), "record %d: %s is not a number", g_record, what);
    return v;
}
static vec inputs(const char* label, size_t count) {
    expect_label(label);
    vec v(count);
    for (uint64_t& x : v) x = input(label);
    return v;
}
static void expect(const char* what, size_t at, uint64_t word) {
    uint64_t v = 0;
    const bool ok = number(&v);
    CHECK(ok && v == word, "record %d: %s word %zu is %llu, the record has %llu", g_record, what, at, (unsigned long long)word, (unsigned long long)v);
}
static void expect_pairs(const char* label, const std::vector<agx::shoup_pair>& pairs) {
    expect_label(label);
    for (size_t k = 0; k < pairs.size(); ++k) expect(label, 2 * k, pairs[k].w), expect(label, 2 * k + 1, pairs[k].p);
}

static int check_golden(const char* path) {
    g_golden = std::fopen(path, "r");
    if (!g_golden) {
        std::printf("cannot read %s\n", path);
        return 2;
    }
    char w[64];
    while (next_word(w)) {
        ++g_record;
        CHECK(!std::strcmp(w, "record"), "record %d: read '%s' where 'record' belongs", g_record, w);
        expect("index", 0, (uint64_t)g_record);
        expect_label("src");
        const uint64_t S = input("S");
        if (S < 1 || S > 16) break;
        const vec src = [&] { vec v(S); for (uint64_t& x : v) x = input("src"); return v; }();
        expect_label("dst");
        const uint64_t T = input("T");
        if (T < 1 || T > 64) break;
        const vec dst = [&] { vec v(T); for (uint64_t& x : v) x = input("dst"); return v; }();
        const vec n_inv = inputs("n_inv", S), w1n = inputs("w1n", S);
        expect_label("t");
        const uint64_t t = input("t");
        expect_label("m");
        const uint64_t m = input("m");
        agx::basis_image b;
        const agx::basis_fault fault = agx::prepare_basis_image(b, {src.data(), (uint32_t)S, dst.data(), (uint32_t)T, n_inv.data(), w1n.data(), t, m});
        expect_label("status");
        expect_label(fault == agx::basis_fault::none ? "ok" : fault == agx::basis_fault::source ? "source" : fault == agx::basis_fault::t ? "t" : "aux");
        if (fault != agx::basis_fault::none) continue;      // a refusal is recorded as a refusal: nothing is promised about the image
        expect_pairs("dinv", b.dinv);
        expect_pairs("mat", b.mat);
        expect_pairs("dall", b.dall);
        expect_label("legal");
        expect("legal", 0, b.moddown_legal ? 1 : 0);
        expect_pairs("sn", b.sn);
        expect_pairs("sw", b.sw);
        expect_pairs("down_mat", b.down_mat);
        expect_pairs("round_src", b.round_src);
        expect_label("round_dst");
        for (size_t j = 0; j < b.round_dst.size(); ++j) expect("round_dst", j, b.round_dst[j]);
        if (!m) continue;
        expect_pairs("aux_row", b.aux_row);
        expect_pairs("aux_corr_exact", b.aux_corr_exact);
        expect_pairs("aux_mdinv", b.aux_mdinv);
        expect_pairs("aux_mmat", b.aux_mmat);
        expect_pairs("aux_corr_mont", b.aux_corr_mont);
        expect_pairs("k_exact", {b.k_exact});
        expect_pairs("k_mont", {b.k_mont});
    }
    const bool whole = std::feof(g_golden) != 0;
    std::fclose(g_golden);
    if (!whole || g_record < 0) {
        std::printf("%s: record %d does not parse\n", path, g_record);
        return 2;
    }
    return 0;
}

static vec primes(uint32_t bits, uint32_t n, uint32_t count) {
    vec p = agx::find_ntt_primes(bits, n, count);
    CHECK(p.size() == count, "find_ntt_primes(%u, %u, %u) found %zu", bits, n, count, p.size());
    return p;
}
static vec slice(const vec& v, size_t lo, size_t hi) { return vec(v.begin() + lo, v.begin() + hi); }

int main(int argc, char** argv) {
    if (argc != 2) {
        std::printf("usage: basis_selftest tests/golden/basis_constants.txt\n");
        return 2;
    }
    const struct {
        uint32_t bits, n;
    } classes[] = {{17, 8}, {30, 64}, {60, 4096}, {62, 1024}};
    for (const auto& c : classes) {
        const vec p = primes(c.bits, c.n, 17);
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
        CHECK(refused({p[0], p[1], p[0]}, p), "%u-bit: equal source moduli accepted", c.bits);
        CHECK(refused({p[3], p[3]}, {p[0]}), "%u-bit: a source given twice accepted", c.bits);
        vec sixteen_and_one = slice(p, 0, 16);
        sixteen_and_one[15] = p[0];
        CHECK(refused(sixteen_and_one, p), "%u-bit: S = 16 with the first modulus repeated accepted", c.bits);
    }
    // mixed widths: a 30-bit source lifted under 62-bit targets and the other way round, and the widths of one RNS chain together
    const vec mixed = {primes(60, 1024, 1)[0], primes(30, 1024, 1)[0], primes(61, 1024, 1)[0], primes(30, 1024, 2)[1], primes(62, 1024, 1)[0],
                       primes(17, 8, 1)[0]};
    check_constants("mixed widths, all -> all", mixed, mixed);
    check_conversion("mixed widths, [30, 61] -> all", {mixed[1], mixed[2]}, mixed, 500);
    check_conversion("mixed widths, [62, 17, 30] -> all", {mixed[4], mixed[5], mixed[3]}, mixed, 500);
    check_conversion("mixed widths, [17] -> all", {mixed[5]}, mixed, 500);
    selftest_section("basis_constants");
    if (int rc = check_golden(argv[1])) return rc;
    return selftest_report("golden");
}
