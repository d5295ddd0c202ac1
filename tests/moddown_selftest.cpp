// moddown_selftest.cpp -- agx::prepare_basis_image (csrc/host_math.cpp), the host side of agx_ntt_basis_mod_down, against brute force in unsigned __int128.
// Stand-alone: built from this file, tests/selftest.hpp and host_math.cpp by tests/test_selftests.py with -fsanitize=address,undefined; no HIP, no plan.
//   * dall[j] D = 1 (mod q_j) with D taken factor by factor in another order than the builder takes it, dall[j] < q_j, its quotient = floor(w 2^64 / q);
//   * sn[i] = n^-1 D_i^-1 and sw[i] = w1n D_i^-1 (mod q_i), reduced, with their quotients; sn[i] n D_i = 1 (mod q_i) closes the loop on n^-1;
//   * where S D fits 128 bits, ModDown itself in exact integers: X = D Y + V' (V' any CRT value of the sources) gives (a_j - V) D^-1 = Y - u (mod q_j)
//     with u = V / D below S;
//   * S = 1, 2, 16 and what lies between, 17-, 30-, 60- and 62-bit-class primes and mixtures of them;
//   * a target that is a source modulus: reported (false, that entry {0, 0}, every other entry still right), not crashed on.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../agilex-ntt_amd/csrc/host_math.hpp"
#include "selftest.hpp"

// D mod m (skip == S) or D_skip mod m, from the last factor to the first (the builder goes first to last)
static uint64_t d_mod_brute(const std::vector<uint64_t>& src, size_t skip, uint64_t m) {
    u128 r = 1 % m;
    for (size_t k = src.size(); k-- > 0;)
        if (k != skip) r = r * (u128)(src[k] % m) % m;
    return (uint64_t)r;
}

// a request with t = 1 and no m, and its image
struct built {
    bool ok;
    std::vector<uint64_t> n_inv, w1n;
    agx::basis_image img;
};
// n: the transform size whose n^-1 the constants carry; w1n: any residue stands for inv_twiddle[1] n^-1
static built build(const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, uint32_t n) {
    const size_t S = src.size(), T = dst.size();
    built b{false, std::vector<uint64_t>(S), std::vector<uint64_t>(S), {}};
    for (size_t i = 0; i < S; ++i) {
        CHECK(agx::inv_mod_euclid(n % src[i], src[i], &b.n_inv[i]), "n has no inverse modulo an odd prime");
        b.w1n[i] = next64() % src[i];
    }
    b.ok = agx::prepare_basis_image(b.img, {src.data(), (uint32_t)S, dst.data(), (uint32_t)T, b.n_inv.data(), b.w1n.data()}) == agx::basis_fault::none;
    if (b.ok) CHECK(b.img.sn.size() == S && b.img.sw.size() == S && b.img.dall.size() == T, "sizes [S], [T]: every entry must be written");
    return b;
}

static void check_constants(const char* what, const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, uint32_t n, bool expect_all) {
    const size_t S = src.size(), T = dst.size();
    const built b = build(src, dst, n);
    CHECK(b.ok, "%s: basis refused", what);
    if (!b.ok) return;
    CHECK(b.img.moddown_legal == expect_all, "%s: reported %d, expected %d", what, (int)b.img.moddown_legal, (int)expect_all);
    for (size_t i = 0; i < S; ++i) {
        const uint64_t q = src[i], di = d_mod_brute(src, i, q);
        CHECK(b.img.sn[i].w < q && b.img.sw[i].w < q, "%s: scaled constants of source %zu not reduced", what, i);
        CHECK(mulmod(mulmod(b.img.sn[i].w, n % q, q), di, q) == 1 % q, "%s: sn[%zu] n D_i != 1", what, i);
        CHECK(b.img.sn[i].w == mulmod(b.n_inv[i], b.img.dinv[i].w, q), "%s: sn[%zu]", what, i);
        CHECK(mulmod(b.img.sw[i].w, di, q) == b.w1n[i], "%s: sw[%zu] D_i != w1n", what, i);
        CHECK(b.img.sn[i].p == (uint64_t)(((u128)b.img.sn[i].w << 64) / q), "%s: quotient of sn[%zu]", what, i);
        CHECK(b.img.sw[i].p == (uint64_t)(((u128)b.img.sw[i].w << 64) / q), "%s: quotient of sw[%zu]", what, i);
    }
    for (size_t j = 0; j < T; ++j) {
        const uint64_t q = dst[j], d = d_mod_brute(src, S, q);
        bool is_source = false;
        for (size_t k = 0; k < S; ++k) is_source |= src[k] == q;
        if (is_source) {
            CHECK(d == 0 && b.img.dall[j].w == 0 && b.img.dall[j].p == 0, "%s: target %zu is a source but has constants", what, j);
            continue;
        }
        CHECK(b.img.dall[j].w < q, "%s: dall[%zu] not reduced", what, j);
        CHECK(mulmod(b.img.dall[j].w, d, q) == 1 % q, "%s: dall[%zu] is not the inverse of D", what, j);
        CHECK(b.img.dall[j].p == (uint64_t)(((u128)b.img.dall[j].w << 64) / q), "%s: quotient of dall[%zu]", what, j);
    }
}

// ModDown in exact integers; needs S D < 2^128 and the quotient Y kept small enough that D Y + S D fits too
static void check_mod_down(const char* what, const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, uint32_t n, int random_values) {
    const size_t S = src.size(), T = dst.size();
    const built b = build(src, dst, n);
    CHECK(b.ok && b.img.moddown_legal, "%s: refused", what);
    if (!b.ok || !b.img.moddown_legal) return;
    u128 D = 1;
    std::vector<u128> Di(S, 1);
    for (size_t i = 0; i < S; ++i) {
        D *= src[i];
        for (size_t k = 0; k < S; ++k)
            if (k != i) Di[i] *= src[k];
    }
    const u128 room = (~(u128)0 / D) - S - 1;      // quotients below this keep D Y + V inside 128 bits
    std::vector<u128> rs = {0, 1, D - 1, D / 2, D / 2 + 1};
    for (int k = 0; k < random_values; ++k) rs.push_back(next128() % D);
    for (const u128 r : rs) {
        const u128 Y = room ? next128() % (room < ((u128)1 << 62) ? room : ((u128)1 << 62)) : 0, X = D * Y + r;
        // the sources see r; the scaled inverse writes y_i = p_i D_i^-1 = (p_i n) (n^-1 D_i^-1): formed through sn to tie the constant in
        u128 V = 0;
        std::vector<uint64_t> y(S);
        for (size_t i = 0; i < S; ++i) {
            const uint64_t q = src[i];
            y[i] = mulmod(mulmod((uint64_t)(r % q), n % q, q), b.img.sn[i].w, q);
            CHECK(y[i] == mulmod((uint64_t)(r % q), b.img.dinv[i].w, q), "%s: the scaled inverse constant does not give y_%zu", what, i);
            V += (u128)y[i] * Di[i];
        }
        CHECK(V % D == r, "%s: V is not congruent to the sources' value", what);
        const u128 u = V / D;
        CHECK(u < S, "%s: u = V / D is not below S", what);
        for (size_t j = 0; j < T; ++j) {
            const uint64_t q = dst[j];
            u128 acc = 0;
            for (size_t i = 0; i < S; ++i) acc += (u128)y[i] * b.img.mat[j * S + i].w;
            const uint64_t a = (uint64_t)(X % q), v = (uint64_t)(acc % q);
            const uint64_t got = mulmod((a + q - v) % q, b.img.dall[j].w, q);
            const uint64_t want = (uint64_t)((Y % q + q - (uint64_t)(u % q)) % q);      // floor(X / D) - u
            CHECK(got == want, "%s: target %zu", what, j);
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
    g_rng = 0x13198A2E03707344ull;
    const struct {
        uint32_t bits, n;
    } classes[] = {{17, 8}, {30, 64}, {60, 4096}, {62, 1024}};
    for (const auto& c : classes) {
        const std::vector<uint64_t> p = primes(c.bits, c.n, 17);
        if (p.size() != 17) continue;
        char what[96];
        for (size_t S : {(size_t)1, (size_t)2, (size_t)3, (size_t)5, (size_t)16}) {
            std::snprintf(what, sizeof what, "%u-bit, S = %zu -> the others", c.bits, S);
            check_constants(what, slice(p, 17 - S, 17), slice(p, 0, 17 - S), c.n, true);      // ModDown: disjoint ranges
            std::snprintf(what, sizeof what, "%u-bit, S = %zu -> all 17", c.bits, S);
            check_constants(what, slice(p, 0, S), p, c.n, false);                               // targets that are sources: reported
            std::snprintf(what, sizeof what, "%u-bit, S = %zu, sources below targets", c.bits, S);
            check_constants(what, slice(p, 0, S), slice(p, S, 17), c.n, true);
        }
        check_constants("one target that is the one source", {p[3]}, {p[3]}, c.n, false);
        check_constants("last target is the first source", slice(p, 4, 6), slice(p, 0, 5), c.n, false);
        for (size_t S = 1; S <= 16 && S * c.bits + 4 + 8 <= 128; ++S) {
            std::snprintf(what, sizeof what, "mod down, %u-bit, S = %zu", c.bits, S);
            check_mod_down(what, slice(p, 17 - S, 17), slice(p, 0, 17 - S), c.n, 200);
        }
    }
    const std::vector<uint64_t> mixed = {primes(60, 1024, 1)[0], primes(30, 1024, 1)[0], primes(61, 1024, 1)[0], primes(30, 1024, 2)[1], primes(62, 1024, 1)[0],
                                         primes(17, 8, 1)[0]};
    check_constants("mixed widths, [30, 61] -> the rest", {mixed[1], mixed[2]}, {mixed[0], mixed[3], mixed[4], mixed[5]}, 8, true);
    check_mod_down("mixed widths, [30, 61] -> the rest", {mixed[1], mixed[2]}, {mixed[0], mixed[3], mixed[4], mixed[5]}, 8, 500);
    check_mod_down("mixed widths, [17] -> the rest", {mixed[5]}, slice(mixed, 0, 5), 8, 500);
    check_mod_down("mixed widths, [62, 30] -> the rest", {mixed[4], mixed[3]}, {mixed[0], mixed[1], mixed[2], mixed[5]}, 8, 500);
    return selftest_report("moddown_constants");
}
