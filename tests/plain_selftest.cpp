// plain_selftest.cpp -- the host side of agx_ntt_plain_scale_up / _lift / _scale_down against brute force: csrc/plain_arith.hpp, the per-word steps and the very
// text the kernels compile, and the constants of agx::prepare_plain_image (csrc/host_math.cpp).  Stand-alone: built from this file, tests/selftest.hpp,
// plain_arith.hpp, bfv_quotient_arith.hpp, bfv_conv_arith.hpp, inner_reduce.hpp and host_math.cpp by tests/test_plain_selftest.py with
// -fsanitize=address,undefined; no HIP, no plan.
//   Moduli: the arguments (the class edges of tests/modulus_cases.py and the smallest admitted primes), at least 20 distinct odd primes.  L = 1, 2, 3, 5, 16
//   primes of Q from every position of the list, gamma behind them; t = 2, 3, 5, 65536, 65537, 2^61 - 1 and 2^62 - 1 (odd, even, a power of two, composite
//   -- 2^62 - 1 = 3 x 715827883 x 2147483647 --, above every modulus).
//   * the steps: plain_reduce for any 64-bit word; plain_scaled and plain_centred over [0, t) with the words next to every sign change; plain_residue for any
//     magnitude below 2^62 and either sign; plain_round over [0, 2t) x [0, 2 gamma) with both centring edges;
//   * the constants: every word by a product that must give a known residue, every quotient floor(w 2^64 / q); the faults in their order;
//   * one coefficient through these constants and steps as the kernels take it against the contract's formulas in 128-bit arithmetic of their own: U by the
//     wide division it avoids (formed modulo q_i from D m' = k t + r), the lift, and scale_down's m from V mod t and V mod gamma.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../agilex-ntt_amd/csrc/plain_arith.hpp"
#include "../agilex-ntt_amd/csrc/host_math.hpp"
#include "selftest.hpp"

typedef unsigned long long ull;

static uint64_t quotient(uint64_t w, uint64_t q) { return (uint64_t)(((u128)w << 64) / q); }
static uint64_t submod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)(((u128)a % q + q - b % q) % q); }
static uint64_t gcd(uint64_t a, uint64_t b) {
    while (b) {
        const uint64_t r = a % b;
        a = b, b = r;
    }
    return a;
}
// a^-1 mod q for any q > 1 with gcd(a, q) = 1, by a search of its own for small q and Euler's theorem through the library-independent power for primes
static uint64_t powmod(uint64_t a, uint64_t e, uint64_t q) {
    uint64_t r = 1 % q;
    for (a %= q; e; e >>= 1, a = mulmod(a, a, q))
        if (e & 1) r = mulmod(r, a, q);
    return r;
}
static uint64_t prod_mod(const std::vector<uint64_t>& v, size_t skip, uint64_t p) {
    u128 r = 1 % p;
    for (size_t k = v.size(); k-- > 0;)
        if (k != skip) r = r * (u128)(v[k] % p) % p;
    return (uint64_t)r;
}

static void check_steps(uint64_t t, uint64_t gamma, uint64_t q) {
    const uint64_t h = t >> 1, one_p = quotient(1, t);
    const uint64_t words[] = {0, 1, t - 1, t, t + 1, 2 * t - 1, ~(uint64_t)0, (uint64_t)1 << 63, ((uint64_t)1 << 62) - 1, next64(), next64(), next64() % t};
    for (uint64_t m : words) {
        const uint64_t got = agx::plain_reduce(m, one_p, t);
        CHECK(got == m % t, "t=%llu: %llu reduced to %llu", (ull)t, (ull)m, (ull)got);
    }
    const uint64_t d = next64() % t, dp = quotient(d, t);
    const uint64_t residues[] = {0, 1 % t, h, (h + 1) % t, h ? h - 1 : 0, t - 1, t - h, t - h - 1, next64() % t, next64() % t, next64() % t, next64() % t};
    for (uint64_t mp : residues) {
        bool negative = false;
        uint64_t mag = agx::plain_scaled(mp, d, dp, h, t, &negative);
        const uint64_t rho = (uint64_t)(((u128)d * mp + h) % t);
        CHECK(mag < t && negative == (rho > h) && mag == (rho > h ? rho - h : h - rho), "t=%llu: scaled %llu", (ull)t, (ull)mp);
        mag = agx::plain_centred(mp, h, t, &negative);
        const bool upper = 2 * (u128)mp >= t;      // m' >= ceil(t / 2)
        CHECK(negative == upper && mag == (upper ? t - mp : mp) && mag <= (negative ? h : (t - 1) / 2), "t=%llu: centred %llu", (ull)t, (ull)mp);
    }
    const uint64_t cs[] = {0, 1 % q, q - 1, next64() % q, next64() % q};
    for (uint64_t c : cs) {
        const uint64_t cp = quotient(c, q);
        for (uint64_t mag : {(uint64_t)0, (uint64_t)1, q - 1, q, q + 1, t - 1, h, ((uint64_t)1 << 62) - 1, next64() >> 2, next64() % q})
            for (bool negative : {false, true}) {
                const uint64_t got = agx::plain_residue(mag, negative, c, cp, q), p = mulmod(mag % q, c, q);
                CHECK(got < q && got == (negative ? submod(0, p, q) : p), "q=%llu: %c%llu x %llu gave %llu", (ull)q, negative ? '-' : '+', (ull)mag, (ull)c, (ull)got);
            }
    }
    if (gcd(gamma % t, t) != 1) return;
    uint64_t g = 0;
    CHECK(agx::inv_mod_euclid(gamma % t, t, &g) && mulmod(g, gamma % t, t) == 1 % t, "gamma^-1 mod t");
    const uint64_t gp = quotient(g, t), half = gamma >> 1;
    for (uint64_t ag : {(uint64_t)0, (uint64_t)1, half, half + 1, gamma - 1, gamma, gamma + half, gamma + half + 1, 2 * gamma - 1, next64() % (2 * gamma)})
        for (uint64_t at : {(uint64_t)0, (uint64_t)1, t - 1, t, 2 * t - 1, next64() % (2 * t), next64() % (2 * t)}) {
            const uint64_t got = agx::plain_round(at, ag, gamma, g, gp, t), s = ag % gamma;
            // acc_t - centre(s) g mod t
            const uint64_t cg = s > half ? submod(0, mulmod((gamma - s) % t, g, t), t) : mulmod(s % t, g, t);
            CHECK(got < t && got == submod(at % t, cg, t), "t=%llu gamma=%llu: round(%llu, %llu) gave %llu", (ull)t, (ull)gamma, (ull)at, (ull)ag, (ull)got);
        }
}

struct built {
    agx::plain_fault fault;
    agx::plain_image img;
    std::vector<uint64_t> n_inv, w1n;      // the last-stage constants handed in: random residues
};

static built build(const std::vector<uint64_t>& Q, uint64_t gamma, uint64_t t) {
    built b;
    for (uint64_t q : Q) b.n_inv.push_back(1 + next64() % (q - 1)), b.w1n.push_back(next64() % q);
    b.fault = agx::prepare_plain_image(b.img, agx::plain_request{Q.data(), (uint32_t)Q.size(), b.n_inv.data(), b.w1n.data(), gamma, t});
    return b;
}

static void check_constants(const std::vector<uint64_t>& Q, uint64_t gamma, uint64_t t, const built& b) {
    const size_t L = Q.size();
    const agx::plain_image& c = b.img;
    CHECK(c.up.size() == L && c.one.size() == L && c.sn.size() == L && c.sw.size() == L && c.row_t.size() == L && c.row_g.size() == L, "sizes");
    if (g_failures) return;
    CHECK(c.h == t / 2 && c.one_t.w == 1 && c.one_t.p == quotient(1, t), "h and 1 mod t");
    CHECK(c.d_t.w == prod_mod(Q, L, t) && c.d_t.p == quotient(c.d_t.w, t), "D mod t");
    CHECK(c.g_t.w < t && mulmod(c.g_t.w, gamma % t, t) == 1 % t && c.g_t.p == quotient(c.g_t.w, t), "gamma^-1 mod t");
    for (size_t i = 0; i < L; ++i) {
        const uint64_t q = Q[i], qi = prod_mod(Q, i, q), scale = mulmod(gamma % q, t % q, q);      // w Q_i = n^-1 gamma t
        CHECK(c.up[i].w < q && mulmod(c.up[i].w, t % q, q) == 1 % q && c.up[i].p == quotient(c.up[i].w, q), "t^-1 mod q[%zu]", i);
        CHECK(c.one[i].w == 1 && c.one[i].p == quotient(1, q), "1 mod q[%zu]", i);
        CHECK(c.sn[i].w < q && mulmod(c.sn[i].w, qi, q) == mulmod(b.n_inv[i], scale, q) && c.sn[i].p == quotient(c.sn[i].w, q), "sn[%zu] q=%llu", i, (ull)q);
        CHECK(c.sw[i].w < q && mulmod(c.sw[i].w, qi, q) == mulmod(b.w1n[i], scale, q) && c.sw[i].p == quotient(c.sw[i].w, q), "sw[%zu] q=%llu", i, (ull)q);
        // row_t q_i gamma = -1 (mod t), row_g q_i = -1 (mod gamma)
        CHECK(c.row_t[i].w < t && (mulmod(mulmod(c.row_t[i].w, q % t, t), gamma % t, t) + 1) % t == 0 && c.row_t[i].p == quotient(c.row_t[i].w, t), "row_t[%zu]", i);
        CHECK(c.row_g[i].w < gamma && (mulmod(c.row_g[i].w, q % gamma, gamma) + 1) % gamma == 0 && c.row_g[i].p == quotient(c.row_g[i].w, gamma), "row_g[%zu]", i);
    }
}

// one plaintext word as plain_encode_kernel takes it
static std::vector<uint64_t> encode_word(const std::vector<uint64_t>& Q, uint64_t t, const built& b, bool lift, uint64_t m) {
    const agx::plain_image& c = b.img;
    const uint64_t mp = agx::plain_reduce(m, c.one_t.p, t);
    bool negative = false;
    const uint64_t mag = lift ? agx::plain_centred(mp, c.h, t, &negative) : agx::plain_scaled(mp, c.d_t.w, c.d_t.p, c.h, t, &negative);
    std::vector<uint64_t> out(Q.size());
    for (size_t i = 0; i < Q.size(); ++i) {
        const agx::shoup_pair& w = lift ? c.one[i] : c.up[i];
        out[i] = agx::plain_residue(mag, negative, w.w, w.p, Q[i]);
    }
    return out;
}

// U mod q by the wide division the device avoids: U = floor((D m' + h) / t), carried as (quotient mod q, remainder below t) one factor of D at a time:
// if A = k t + r then A f = (k f) t + r f = (k f + floor(r f / t)) t + (r f mod t)
static uint64_t scale_up_mod(const std::vector<uint64_t>& Q, uint64_t t, uint64_t m, uint64_t q) {
    const uint64_t mp = m % t;
    uint64_t k = 0, r = mp;      // m' = 0 t + m'
    for (uint64_t f : Q) {
        const u128 rf = (u128)r * f;
        k = (uint64_t)(((u128)mulmod(k, f % q, q) + (uint64_t)((rf / t) % q)) % q);
        r = (uint64_t)(rf % t);
    }
    return (uint64_t)(((u128)k + ((u128)r + t / 2 >= t ? 1 : 0)) % q);      // + floor((r + h) / t)
}

// one coefficient as the scaled inverse and plain_scale_down_kernel take it: a [L] reduced coefficient words
static uint64_t scale_down_word(const std::vector<uint64_t>& Q, uint64_t gamma, uint64_t t, const built& b, const std::vector<uint64_t>& a) {
    const agx::plain_image& c = b.img;
    uint64_t acc_t = 0, acc_g = 0;
    for (size_t i = 0; i < Q.size(); ++i) {
        // the last stage multiplies by the scaled n^-1 in the place of n^-1: a word a n^-1 becomes a (n^-1 scale)
        const uint64_t y = agx::bfv_shoup(mulmod(a[i], powmod(b.n_inv[i], Q[i] - 2, Q[i]), Q[i]), c.sn[i].w, c.sn[i].p, Q[i]);
        acc_t = agx::quot_accumulate(acc_t, y, c.row_t[i].w, c.row_t[i].p, t, t << 1);
        acc_g = agx::quot_accumulate(acc_g, y, c.row_g[i].w, c.row_g[i].p, gamma, gamma << 1);
    }
    return agx::plain_round(acc_t, acc_g, gamma, c.g_t.w, c.g_t.p, t);
}

// the contract's formula in modular arithmetic of its own: V mod p = sum_i y_i (Q_i mod p); *s_gamma_out: s_gamma
static uint64_t contract_scale_down(const std::vector<uint64_t>& Q, uint64_t gamma, uint64_t t, const std::vector<uint64_t>& a, uint64_t* s_gamma_out) {
    const size_t L = Q.size();
    std::vector<uint64_t> y(L);
    for (size_t i = 0; i < L; ++i)
        y[i] = mulmod(a[i], mulmod(mulmod(gamma % Q[i], t % Q[i], Q[i]), powmod(prod_mod(Q, i, Q[i]), Q[i] - 2, Q[i]), Q[i]), Q[i]);
    auto s_mod = [&](uint64_t p) {      // (-V D^-1) mod p, p coprime to D
        u128 v = 0;
        for (size_t i = 0; i < L; ++i) v = (v + (u128)(y[i] % p) * prod_mod(Q, i, p)) % p;
        uint64_t dinv = 0;
        (void)agx::inv_mod_euclid(prod_mod(Q, L, p), p, &dinv);
        return submod(0, mulmod((uint64_t)v, dinv, p), p);
    };
    const uint64_t s_t = s_mod(t), s_g = s_mod(gamma);
    *s_gamma_out = s_g;
    uint64_t ginv = 0;
    (void)agx::inv_mod_euclid(gamma % t, t, &ginv);
    const uint64_t diff = s_g > (gamma >> 1) ? (uint64_t)(((u128)s_t + (gamma - s_g) % t) % t) : submod(s_t, s_g % t, t);      // s_t - centre(s_gamma)
    return mulmod(diff, ginv, t);
}

static void check_words(const std::vector<uint64_t>& Q, uint64_t gamma, uint64_t t, const built& b, int values) {
    const size_t L = Q.size();
    const uint64_t ms[] = {0, 1, t - 1, t, t / 2, t / 2 + 1, (t + 1) / 2, (t + 1) / 2 - 1, ~(uint64_t)0};
    for (int k = 0; k < values; ++k) {
        const uint64_t m = k < 9 ? ms[k] : next64();
        const std::vector<uint64_t> up = encode_word(Q, t, b, false, m), lifted = encode_word(Q, t, b, true, m);
        const uint64_t mp = m % t;
        for (size_t i = 0; i < L; ++i) {
            const uint64_t q = Q[i];
            CHECK(up[i] == scale_up_mod(Q, t, m, q), "L=%zu t=%llu m=%llu: scale_up under %llu gave %llu", L, (ull)t, (ull)m, (ull)q, (ull)up[i]);
            const uint64_t want = 2 * (u128)mp >= t ? submod(mp, t, q) : mp % q;
            CHECK(lifted[i] == want, "L=%zu t=%llu m=%llu: lift under %llu gave %llu", L, (ull)t, (ull)m, (ull)q, (ull)lifted[i]);
        }
    }
    const uint64_t half = gamma >> 1;
    const uint64_t edges[] = {half, half + 1, 0, 1, gamma - 1};
    for (int k = 0; k < values; ++k) {
        std::vector<uint64_t> a(L);
        for (size_t i = 0; i < L; ++i) a[i] = k == 0 ? 0 : k == 1 ? Q[i] - 1 : next64() % Q[i];
        uint64_t s_g = 0;
        if (k >= 2 && k < 7 && t % gamma) {
            // choose a_0 for a wanted s_gamma: s_gamma is affine in a_0 with slope -(gamma t Q_0^-1 mod q_0) q_0^-1 mod gamma; search a few words instead of
            // solving (y_0 is reduced modulo q_0 first, so the map is not linear over the integers): small gamma only
            if (gamma < 4096)
                for (uint64_t trial = 0; trial < 4 * gamma && ((void)contract_scale_down(Q, gamma, t, a, &s_g), s_g != edges[k - 2]); ++trial) a[0] = (a[0] + 1) % Q[0];
        }
        const uint64_t want = contract_scale_down(Q, gamma, t, a, &s_g), got = scale_down_word(Q, gamma, t, b, a);
        CHECK(got == want && got < t, "L=%zu gamma=%llu t=%llu s_gamma=%llu: %llu, not %llu", L, (ull)gamma, (ull)t, (ull)s_g, (ull)got, (ull)want);
    }
}

int main(int argc, char** argv) {
    g_rng = 0xA4093822299F31D0ull;
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
    const uint64_t ts[] = {2, 3, 5, 65536, 65537, (1ull << 61) - 1, (1ull << 62) - 1};
    for (size_t k = 0; k < M; ++k)
        for (uint64_t t : ts) check_steps(t, moduli[k], moduli[(k + 1) % M]);
    selftest_section("plain_arith");
    const size_t counts[] = {1, 2, 3, 5, 16};
    for (size_t L : counts)
        for (size_t first = 0; first < M; ++first) {
            std::vector<uint64_t> Q;
            for (size_t k = 0; k < L; ++k) Q.push_back(moduli[(first + k) % M]);
            const uint64_t gamma = moduli[(first + L) % M];
            for (uint64_t t : ts) {
                const built b = build(Q, gamma, t);
                bool shares = gcd(gamma, t) != 1;
                for (uint64_t q : Q) shares |= gcd(q, t) != 1;
                if (shares) {      // 65537 and 2^61 - 1 are admitted primes at some sizes; 2^62 - 1 has small factors
                    CHECK(b.fault == agx::plain_fault::t_source || b.fault == agx::plain_fault::t_gamma, "L=%zu t=%llu: a shared factor was accepted", L, (ull)t);
                    continue;
                }
                CHECK(b.fault == agx::plain_fault::none, "L=%zu gamma=%llu t=%llu: refused", L, (ull)gamma, (ull)t);
                if (b.fault != agx::plain_fault::none) continue;
                check_constants(Q, gamma, t, b);
                check_words(Q, gamma, t, b, 14);
            }
            // the faults in their order: equal moduli in Q, gamma in Q, t out of range, q_i | t, gamma | t
            std::vector<uint64_t> bad = Q;
            if (L >= 2) {
                bad[L - 1] = Q[0];
                CHECK(build(bad, gamma, 0).fault == agx::plain_fault::source, "two equal moduli were accepted");
            }
            CHECK(build(Q, Q[L - 1], 0).fault == agx::plain_fault::gamma, "gamma in Q was accepted");
            for (uint64_t t : {(uint64_t)0, (uint64_t)1, (uint64_t)1 << 62, ~(uint64_t)0})
                CHECK(build(Q, gamma, t).fault == agx::plain_fault::t_range, "t = %llu was accepted", (ull)t);
            if (Q[L - 1] < (1ull << 61)) CHECK(build(Q, gamma, 2 * Q[L - 1]).fault == agx::plain_fault::t_source, "q | t was accepted");
            if (gamma < (1ull << 61)) CHECK(build(Q, gamma, 2 * gamma).fault == agx::plain_fault::t_gamma, "gamma | t was accepted");
            if (Q[0] < (1ull << 30) && gamma < (1ull << 30)) CHECK(build(Q, gamma, Q[0] * gamma).fault == agx::plain_fault::t_source, "q | t comes before gamma | t");
        }
    std::printf("moduli: %zu\n", M);
    return selftest_report("plain");
}
