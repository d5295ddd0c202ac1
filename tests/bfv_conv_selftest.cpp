// bfv_conv_selftest.cpp -- the host side of agx_ntt_basis_extend_exact and agx_ntt_basis_extend_mont against brute force: csrc/bfv_conv_arith.hpp, the per-word
// steps and the very text the kernel compiles, and agx::prepare_basis_image (csrc/host_math.cpp).  Stand-alone: built from this file, tests/selftest.hpp,
// bfv_conv_arith.hpp, inner_reduce.hpp and host_math.cpp by tests/test_selftests.py with -fsanitize=address,undefined; no HIP, no plan.
//   Moduli: the arguments (the class edges of tests/modulus_cases.py: the primes next to 2^31, 2^60, 2^61 and 2^62, those next to 2^60 - 2^28, the
//   smallest admitted primes), at least 20 distinct odd primes.  S = 1, 2 and 16 sources taken from every position of the list, three targets behind them
//   and the auxiliary prime m behind those: m comes from every class, tiny ones included.
//   * the steps: bfv_reduce_lazy over [0, 4m); bfv_shoup for any 64-bit word; bfv_alpha at and next to the wrap; bfv_centre at both edges ((m - 1) / 2 stays,
//     (m + 1) / 2 becomes -(m - 1) / 2); bfv_correct over [0, 2q) with either sign, the result below q;
//   * the constants: every word against products taken factor by factor in another order, every quotient floor(w 2^64 / q); m equal to a source or a target
//     is refused;
//   * both conversions through these constants and steps, V never formed: V mod p = sum_i y_i (D_i mod p) mod p for any p.  Exact: the y_i and an alpha in
//     [-(m - 1) / 2, (m - 1) / 2] are chosen, both edges among them, r = (V - alpha D) mod m, lazy words; the outputs must be (V - alpha D) mod q_j.  Mont:
//     (V + alpha D) = 0 (mod m) and the outputs times m are (V + alpha D) mod q_j; where m S D fits 123 bits, W = (V + alpha D) / m in exact integers is X or
//     X - D inside its bounds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../agilex-ntt_amd/csrc/bfv_conv_arith.hpp"
#include "../agilex-ntt_amd/csrc/host_math.hpp"
#include "selftest.hpp"

typedef __int128 i128;
typedef unsigned long long ull;

// D mod p (skip == S) or D_skip mod p, from the last factor to the first (the builder goes first to last)
static uint64_t d_mod_brute(const std::vector<uint64_t>& src, size_t skip, uint64_t p) {
    u128 r = 1 % p;
    for (size_t k = src.size(); k-- > 0;)
        if (k != skip) r = r * (u128)(src[k] % p) % p;
    return (uint64_t)r;
}

static uint64_t quotient(uint64_t w, uint64_t q) { return (uint64_t)(((u128)w << 64) / q); }
static uint64_t submod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)(((u128)a + q - b % q) % q); }

static void check_steps(uint64_t q) {
    const uint64_t ws[] = {0, 1 % q, q / 2, (q / 2 + 1) % q, q - 1, next64() % q, next64() % q};
    for (uint64_t v : {(uint64_t)0, q - 1, q, q + 1, 2 * q - 1, 2 * q, 3 * q, 4 * q - 1, next64() % (4 * q), next64() % (4 * q)}) {
        if (v >= 4 * q) continue;
        CHECK(agx::bfv_reduce_lazy(v, q) == v % q, "q=%llu: %llu", (ull)q, (ull)v);
    }
    for (uint64_t w : ws) {
        const uint64_t wp = quotient(w, q);
        for (uint64_t y : {(uint64_t)0, (uint64_t)1, q - 1, q, ~(uint64_t)0, ~(uint64_t)0 - 1, (uint64_t)1 << 63, next64(), next64(), next64() % q, ((uint64_t)1 << 61) - 1}) {
            const uint64_t got = agx::bfv_shoup(y, w, wp, q);
            CHECK(got == (uint64_t)((u128)y * w % q), "q=%llu: %llu x %llu gave %llu", (ull)q, (ull)y, (ull)w, (ull)got);
        }
    }
    // alpha and its centring: q plays m
    const uint64_t half = q >> 1;
    for (uint64_t k : ws) {
        const uint64_t kp = quotient(k, q);
        for (uint64_t vm : ws)
            for (uint64_t r : {vm, (vm + 1) % q, (vm + q - 1) % q, (uint64_t)0, q - 1, next64() % q}) {
                const uint64_t a = agx::bfv_alpha(vm, r, k, kp, q);
                CHECK(a == mulmod(submod(vm, r, q), k, q) && a < q, "m=%llu: (%llu - %llu) %llu gave %llu", (ull)q, (ull)vm, (ull)r, (ull)k, (ull)a);
            }
    }
    for (uint64_t a : {(uint64_t)0, 1 % q, half ? half - 1 : 0, half, (half + 1) % q, (half + 2) % q, q - 1, next64() % q}) {
        bool negative = false;
        const uint64_t mag = agx::bfv_centre(a, q, &negative);
        CHECK(negative == (a > half) && mag == (a > half ? q - a : a) && mag <= half, "m=%llu: centre(%llu)", (ull)q, (ull)a);
    }
    bool negative = true;
    CHECK(agx::bfv_centre(half, q, &negative) == half && !negative, "the upper edge");
    if (q > 1) CHECK(agx::bfv_centre(half + 1, q, &negative) == half && negative, "the lower edge");
    // the correction: mag is a residue of another modulus, up to 2^61 - 1
    for (uint64_t c : ws) {
        const uint64_t cp = quotient(c, q);
        for (uint64_t acc : {(uint64_t)0, q - 1, q, q + 1, 2 * q - 1, next64() % (2 * q), next64() % (2 * q)})
            for (uint64_t mag : {(uint64_t)0, (uint64_t)1, q - 1, q, q + 1, ((uint64_t)1 << 61) - 1, next64() >> 3, next64() % q})
                for (int sign = 0; sign < 2; ++sign) {
                    const uint64_t got = agx::bfv_correct(acc, mag, sign != 0, c, cp, q), p = (uint64_t)((u128)mag * c % q);
                    const uint64_t want = sign ? (uint64_t)(((u128)acc + p) % q) : submod(acc % q, p, q);
                    CHECK(got == want && got < q, "q=%llu: %llu %c %llu x %llu gave %llu", (ull)q, (ull)acc, sign ? '+' : '-', (ull)mag, (ull)c, (ull)got);
                }
    }
}

// the image of a request with t = 1 and the auxiliary modulus m; the last-stage constants, which the conversions do not read, are ones
struct built {
    bool ok = false;
    agx::basis_image img;
};

static built build(const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, uint64_t m) {
    const std::vector<uint64_t> one(src.size(), 1);
    built b;
    b.ok = agx::prepare_basis_image(b.img, {src.data(), (uint32_t)src.size(), dst.data(), (uint32_t)dst.size(), one.data(), one.data(), 1, m}) == agx::basis_fault::none;
    return b;
}

static void check_constants(const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, uint64_t m, const built& b) {
    const size_t S = src.size(), T = dst.size();
    const agx::basis_image& c = b.img;
    CHECK(c.aux_row.size() == S && c.aux_mdinv.size() == S, "sizes [S]");
    CHECK(c.aux_corr_exact.size() == T && c.aux_corr_mont.size() == T, "sizes [T]");
    CHECK(c.aux_mmat.size() == T * S, "sizes [T][S]");
    const uint64_t Dm = d_mod_brute(src, S, m);
    CHECK(c.k_exact.w < m && mulmod(c.k_exact.w, Dm, m) == 1 % m, "S=%zu m=%llu: k_exact", S, (ull)m);
    CHECK(c.k_mont.w < m && (c.k_exact.w + c.k_mont.w) % m == 0, "S=%zu m=%llu: k_mont", S, (ull)m);
    CHECK(c.k_exact.p == quotient(c.k_exact.w, m) && c.k_mont.p == quotient(c.k_mont.w, m), "quotients of k");
    for (size_t i = 0; i < S; ++i) {
        const uint64_t q = src[i];
        CHECK(c.aux_row[i].w == d_mod_brute(src, i, m) && c.aux_row[i].p == quotient(c.aux_row[i].w, m), "S=%zu m=%llu: row[%zu]", S, (ull)m, i);
        CHECK(c.aux_mdinv[i].w < q && mulmod(c.aux_mdinv[i].w, d_mod_brute(src, i, q), q) == m % q, "S=%zu m=%llu: mdinv[%zu]", S, (ull)m, i);
        CHECK(c.aux_mdinv[i].p == quotient(c.aux_mdinv[i].w, q), "quotient of mdinv[%zu]", i);
    }
    for (size_t j = 0; j < T; ++j) {
        const uint64_t q = dst[j], Dq = d_mod_brute(src, S, q);
        CHECK(c.aux_corr_exact[j].w == Dq && c.aux_corr_exact[j].p == quotient(Dq, q), "S=%zu: corr_exact[%zu]", S, j);
        CHECK(c.aux_corr_mont[j].w < q && (mulmod(c.aux_corr_mont[j].w, m % q, q) + Dq) % q == 0, "S=%zu m=%llu: corr_mont[%zu]", S, (ull)m, j);
        CHECK(c.aux_corr_mont[j].p == quotient(c.aux_corr_mont[j].w, q), "quotient of corr_mont[%zu]", j);
        for (size_t i = 0; i < S; ++i) {
            const size_t at = j * S + i;
            CHECK(c.aux_mmat[at].w < q && mulmod(c.aux_mmat[at].w, m % q, q) == d_mod_brute(src, i, q), "S=%zu m=%llu: mmat[%zu][%zu]", S, (ull)m, j, i);
            CHECK(c.aux_mmat[at].p == quotient(c.aux_mmat[at].w, q), "quotient of mmat[%zu][%zu]", j, i);
        }
    }
}

static int bits_of(u128 v) {
    int b = 0;
    while (v) ++b, v >>= 1;
    return b;
}

// what the kernel computes for one coefficient from these constants and steps; the accumulators are handed over anywhere in their lazy range [0, 2q)
static std::vector<uint64_t> kernel_word(const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, uint64_t m, const built& b, bool exact,
                                         const std::vector<uint64_t>& x, uint64_t xaux) {
    const size_t S = src.size(), T = dst.size();
    const agx::basis_image& c = b.img;
    std::vector<uint64_t> y(S), out(T);
    uint64_t vm = 0;
    for (size_t i = 0; i < S; ++i) {
        y[i] = agx::bfv_shoup(x[i], exact ? b.img.dinv[i].w : c.aux_mdinv[i].w, exact ? b.img.dinv[i].p : c.aux_mdinv[i].p, src[i]);
        vm = (uint64_t)(((u128)vm + agx::bfv_shoup(y[i], c.aux_row[i].w, c.aux_row[i].p, m)) % m);
    }
    const uint64_t r = exact ? agx::bfv_reduce_lazy(xaux, m) : 0;
    bool negative = false;
    const uint64_t mag = agx::bfv_centre(agx::bfv_alpha(vm, r, exact ? c.k_exact.w : c.k_mont.w, exact ? c.k_exact.p : c.k_mont.p, m), m, &negative);
    for (size_t j = 0; j < T; ++j) {
        const uint64_t q = dst[j];
        uint64_t acc = 0;
        for (size_t i = 0; i < S; ++i) {
            const size_t at = j * S + i;
            acc = (uint64_t)(((u128)acc + agx::bfv_shoup(y[i], exact ? b.img.mat[at].w : c.aux_mmat[at].w, exact ? b.img.mat[at].p : c.aux_mmat[at].p, q)) % q);
        }
        if (next64() & 1) acc += q;
        out[j] = agx::bfv_correct(acc, mag, negative, exact ? c.aux_corr_exact[j].w : c.aux_corr_mont[j].w, exact ? c.aux_corr_exact[j].p : c.aux_corr_mont[j].p, q);
    }
    return out;
}

// V mod p for V = sum_i y_i D_i
static uint64_t v_mod(const std::vector<uint64_t>& src, const std::vector<uint64_t>& y, uint64_t p) {
    u128 v = 0;
    for (size_t i = 0; i < src.size(); ++i) v = (v + (u128)(y[i] % p) * d_mod_brute(src, i, p)) % p;
    return (uint64_t)v;
}

static void check_conversions(const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, uint64_t m, const built& b, int values) {
    const size_t S = src.size(), T = dst.size();
    const uint64_t half = m >> 1;
    std::vector<i128> alphas = {0, 1, -1, (i128)half, -(i128)half, (i128)half - 1, -((i128)half - 1)};
    for (int k = 0; k < values; ++k) alphas.push_back((i128)(next64() % m) - (i128)half);
    for (const i128 alpha : alphas) {
        if (alpha > (i128)half || alpha < -(i128)half) continue;
        // exact: choose the y_i, then x_i = y_i D_i mod q_i spread over [0, 4 q_i) and r = (V - alpha D) mod m spread over [0, 4m)
        std::vector<uint64_t> y(S), x(S);
        for (size_t i = 0; i < S; ++i) {
            y[i] = alpha == 0 && i == 0 ? src[i] - 1 : next64() % src[i];
            x[i] = mulmod(y[i], d_mod_brute(src, i, src[i]), src[i]) + (next64() & 3) * src[i];
        }
        auto minus_alpha_d = [&](uint64_t p) {      // (V - alpha D) mod p
            const uint64_t a = (uint64_t)(alpha < 0 ? -alpha : alpha) % p, ad = mulmod(a, d_mod_brute(src, S, p), p), v = v_mod(src, y, p);
            return alpha < 0 ? (uint64_t)(((u128)v + ad) % p) : submod(v, ad, p);
        };
        const uint64_t r = minus_alpha_d(m) + (next64() & 3) * m;
        const std::vector<uint64_t> got = kernel_word(src, dst, m, b, true, x, r);
        for (size_t j = 0; j < T; ++j) CHECK(got[j] == minus_alpha_d(dst[j]), "exact S=%zu m=%llu alpha=%lld: target %zu", S, (ull)m, (long long)alpha, j);
    }
    int dbits = 0;
    for (uint64_t q : src) dbits += bits_of(q);
    for (int k = 0; k < values + 4; ++k) {
        std::vector<uint64_t> x(S), y(S);
        for (size_t i = 0; i < S; ++i) {
            const uint64_t xr = k == 0 ? 0 : k == 1 ? src[i] - 1 : k == 2 ? 1 % src[i] : next64() % src[i];
            x[i] = xr + (next64() & 3) * src[i];
            y[i] = mulmod(mulmod(xr, m % src[i], src[i]), b.img.dinv[i].w, src[i]);      // x_i' m D_i^-1 mod q_i
        }
        uint64_t dm_inv = 0;
        CHECK(agx::inv_mod_euclid(d_mod_brute(src, S, m), m, &dm_inv), "D has no inverse modulo m");
        const uint64_t a = mulmod(submod(0, v_mod(src, y, m), m), dm_inv, m);      // (-V D^-1) mod m
        const bool negative = a > half;
        const uint64_t mag = negative ? m - a : a;
        auto plus_alpha_d = [&](uint64_t p) {      // (V + alpha D) mod p
            const uint64_t ad = mulmod(mag % p, d_mod_brute(src, S, p), p), v = v_mod(src, y, p);
            return negative ? submod(v, ad, p) : (uint64_t)(((u128)v + ad) % p);
        };
        CHECK(plus_alpha_d(m) == 0, "mont S=%zu m=%llu: m does not divide V + alpha D", S, (ull)m);
        const std::vector<uint64_t> got = kernel_word(src, dst, m, b, false, x, 0);
        for (size_t j = 0; j < T; ++j) CHECK(mulmod(got[j], m % dst[j], dst[j]) == plus_alpha_d(dst[j]) && got[j] < dst[j], "mont S=%zu m=%llu: target %zu", S, (ull)m, j);
        if (dbits + bits_of(m) + bits_of(S) + 3 > 126 || m <= 2 * S) continue;      // alpha D, m (2W - D) and 2 S D fit a signed 128-bit word
        // exact integers: W = (V + alpha D) / m is X or X - D, -D/2 < W < D/2 + S D / m, and the outputs are its residues
        u128 D = 1, V = 0, X = 0;
        for (uint64_t q : src) D *= q;
        for (size_t i = 0; i < S; ++i) {
            V += (u128)y[i] * (D / src[i]);
            X += (u128)mulmod(x[i] % src[i], b.img.dinv[i].w, src[i]) * (D / src[i]);
        }
        X %= D;
        const i128 num = (i128)V + (negative ? -(i128)mag : (i128)mag) * (i128)D;
        CHECK(num % (i128)m == 0, "V + alpha D is not divisible by m");
        const i128 W = num / (i128)m;
        CHECK(W == (i128)X || W == (i128)X - (i128)D, "mont S=%zu m=%llu: W is neither X nor X - D", S, (ull)m);
        CHECK(2 * W > -(i128)D && (2 * W - (i128)D) * (i128)m < 2 * (i128)S * (i128)D, "mont S=%zu m=%llu: W outside its bounds", S, (ull)m);
        for (size_t j = 0; j < T; ++j) {
            const i128 w = W % (i128)dst[j];
            CHECK(got[j] == (uint64_t)(w < 0 ? w + (i128)dst[j] : w), "mont S=%zu m=%llu: target %zu is not W's residue", S, (ull)m, j);
        }
    }
}

int main(int argc, char** argv) {
    g_rng = 0x082EFA98EC4E6C89ull;
    std::vector<uint64_t> moduli;
    for (int i = 1; i < argc; ++i) {
        const uint64_t q = std::strtoull(argv[i], nullptr, 10);
        if (q < 3 || !(q & 1) || q >= (1ull << 62) || !agx::is_prime_u64(q)) {
            std::printf("not an odd prime in [3, 2^62): %s\n", argv[i]);
            return 2;
        }
        bool seen = false;
        for (uint64_t m : moduli) seen |= m == q;
        if (!seen) moduli.push_back(q);
    }
    if (moduli.size() < 20) {
        std::printf("at least 20 distinct moduli are needed, got %zu\n", moduli.size());
        return 2;
    }
    const size_t M = moduli.size();
    for (uint64_t q : moduli) check_steps(q);
    selftest_section("bfv_conv_arith");
    for (size_t S : {(size_t)1, (size_t)2, (size_t)16})
        for (size_t first = 0; first < M; ++first) {
            std::vector<uint64_t> src, dst;
            for (size_t k = 0; k < S; ++k) src.push_back(moduli[(first + k) % M]);
            for (size_t k = 0; k < 3; ++k) dst.push_back(moduli[(first + S + k) % M]);
            const uint64_t m = moduli[(first + S + 3) % M];
            const built b = build(src, dst, m);
            CHECK(b.ok, "S=%zu m=%llu: refused", S, (ull)m);
            if (!b.ok) continue;
            check_constants(src, dst, m, b);
            check_conversions(src, dst, m, b, 24);
            CHECK(!build(src, dst, src[S - 1]).ok && !build(src, dst, dst[1]).ok, "an auxiliary modulus that is a source's or a target's was accepted");
        }
    std::printf("moduli: %zu\n", M);
    return selftest_report("bfv_conversions");
}
