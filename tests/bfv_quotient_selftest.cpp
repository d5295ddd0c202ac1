// bfv_quotient_selftest.cpp -- the host side of agx_ntt_basis_quotient against brute force: csrc/bfv_quotient_arith.hpp, the per-word steps and the very text
// the kernel compiles, and the quotient's constants of agx::prepare_basis_image (csrc/host_math.cpp).  Stand-alone: built from this file, tests/selftest.hpp,
// bfv_quotient_arith.hpp, bfv_conv_arith.hpp, inner_reduce.hpp and host_math.cpp by tests/test_quotient_selftest.py with -fsanitize=address,undefined; no HIP,
// no plan.
//   Moduli: the arguments (the class edges of tests/modulus_cases.py and the smallest admitted primes), at least 20 distinct odd primes.  K = 1, 2 and 16
//   sources B from every position of the list, the auxiliary prime m behind them and L = 1, 3 or 16 targets Q behind that; t = 1, 2, 65537 and 2^64 - 59.
//   * the steps: quot_accumulate over [0, 2q) for any 64-bit word, the result in [0, 2q) and congruent; quot_residue over [0, q) x [0, 2q);
//   * the constants: every word by a product that must give a known residue, every quotient floor(w 2^64 / q); a request without quot_t leaves them
//     empty; a target equal to a source or to m, and two equal targets, are refused;
//   * one coefficient through these constants and steps as the kernel takes it (the scaled inverses' last stage is one product by the scaled n^-1)
//     against the contract's formula in modular arithmetic of its own: V mod p = sum_i y_i (Q_i mod p), f_j, z_j, W mod p = sum_j z_j (B_j mod p), alpha,
//     out_i = (W - alpha B) mod q_i; the auxiliary word is also chosen so that alpha takes both centring edges, 0 and +-1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../agilex-ntt_amd/csrc/bfv_quotient_arith.hpp"
#include "../agilex-ntt_amd/csrc/host_math.hpp"
#include "selftest.hpp"

typedef unsigned long long ull;

static uint64_t quotient(uint64_t w, uint64_t q) { return (uint64_t)(((u128)w << 64) / q); }
static uint64_t submod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)(((u128)a % q + q - b % q) % q); }
static uint64_t powmod(uint64_t a, uint64_t e, uint64_t q) {
    uint64_t r = 1 % q;
    for (a %= q; e; e >>= 1, a = mulmod(a, a, q))
        if (e & 1) r = mulmod(r, a, q);
    return r;
}
static uint64_t invmod(uint64_t a, uint64_t q) { return powmod(a, q - 2, q); }      // q prime
// prod mod p of the list (skip == size: all of it), from the last factor to the first
static uint64_t prod_mod(const std::vector<uint64_t>& v, size_t skip, uint64_t p) {
    u128 r = 1 % p;
    for (size_t k = v.size(); k-- > 0;)
        if (k != skip) r = r * (u128)(v[k] % p) % p;
    return (uint64_t)r;
}

static void check_steps(uint64_t q) {
    const uint64_t ws[] = {0, 1 % q, q / 2, q - 1, next64() % q, next64() % q};
    for (uint64_t c : ws) {
        const uint64_t cp = quotient(c, q);
        for (uint64_t acc : {(uint64_t)0, q - 1, q, q + 1, 2 * q - 1, next64() % (2 * q)})
            for (uint64_t y : {(uint64_t)0, (uint64_t)1, q - 1, q, ~(uint64_t)0, (uint64_t)1 << 63, next64(), next64() % q, ((uint64_t)1 << 62) - 1}) {
                const uint64_t got = agx::quot_accumulate(acc, y, c, cp, q, q << 1);
                CHECK(got < 2 * q && got % q == (uint64_t)(((u128)y * c + acc) % q), "q=%llu: %llu + %llu x %llu gave %llu", (ull)q, (ull)acc, (ull)y, (ull)c, (ull)got);
            }
    }
    for (uint64_t s : ws)
        for (uint64_t acc : {(uint64_t)0, s, (s + 1) % q, q - 1, q, q + s, 2 * q - 1, next64() % (2 * q)}) {
            const uint64_t got = agx::quot_residue(s, acc, q);
            CHECK(got < q && got == submod(s, acc, q), "q=%llu: %llu - %llu gave %llu", (ull)q, (ull)s, (ull)acc, (ull)got);
        }
}

struct built {
    agx::basis_fault fault;
    agx::basis_image img;
    std::vector<uint64_t> sn, sw, dn, dw;      // the last-stage constants handed in: random residues
    uint64_t an = 0, aw = 0;
};

static built build(const std::vector<uint64_t>& B, const std::vector<uint64_t>& Q, uint64_t m, uint64_t t) {
    built b;
    for (uint64_t q : B) b.sn.push_back(1 + next64() % (q - 1)), b.sw.push_back(next64() % q);
    for (uint64_t q : Q) b.dn.push_back(1 + next64() % (q - 1)), b.dw.push_back(next64() % q);
    b.an = 1 + next64() % (m - 1), b.aw = next64() % m;
    agx::basis_request rq{B.data(), (uint32_t)B.size(), Q.data(), (uint32_t)Q.size(), b.sn.data(), b.sw.data(), 1, m};
    rq.quot_t = t, rq.dst_n_inv = b.dn.data(), rq.dst_w1n = b.dw.data(), rq.aux_n_inv = b.an, rq.aux_w1n = b.aw;
    b.fault = agx::prepare_basis_image(b.img, rq);
    return b;
}

static void check_constants(const std::vector<uint64_t>& B, const std::vector<uint64_t>& Q, uint64_t m, uint64_t t, const built& b) {
    const size_t K = B.size(), L = Q.size();
    const agx::basis_image& c = b.img;
    CHECK(c.quot_dn.size() == L && c.quot_dw.size() == L && c.quot_sn.size() == K + 1 && c.quot_sw.size() == K + 1 && c.quot_mat.size() == L * (K + 1), "sizes");
    if (g_failures) return;
    for (size_t j = 0; j < L; ++j) {
        const uint64_t q = Q[j], ej = prod_mod(Q, j, q);      // w E_j = n^-1 t
        CHECK(c.quot_dn[j].w < q && mulmod(c.quot_dn[j].w, ej, q) == mulmod(b.dn[j], t % q, q), "dn[%zu] q=%llu", j, (ull)q);
        CHECK(c.quot_dw[j].w < q && mulmod(c.quot_dw[j].w, ej, q) == mulmod(b.dw[j], t % q, q), "dw[%zu] q=%llu", j, (ull)q);
        CHECK(c.quot_dn[j].p == quotient(c.quot_dn[j].w, q) && c.quot_dw[j].p == quotient(c.quot_dw[j].w, q), "quotients of dn, dw [%zu]", j);
    }
    for (size_t i = 0; i <= K; ++i) {
        const uint64_t q = i < K ? B[i] : m, scale = mulmod(prod_mod(Q, L, q), i < K ? prod_mod(B, i, q) : 1 % q, q);      // w E D_i = n^-1 t
        CHECK(c.quot_sn[i].w < q && mulmod(c.quot_sn[i].w, scale, q) == mulmod(i < K ? b.sn[i] : b.an, t % q, q), "sn[%zu] q=%llu", i, (ull)q);
        CHECK(c.quot_sw[i].w < q && mulmod(c.quot_sw[i].w, scale, q) == mulmod(i < K ? b.sw[i] : b.aw, t % q, q), "sw[%zu] q=%llu", i, (ull)q);
        CHECK(c.quot_sn[i].p == quotient(c.quot_sn[i].w, q) && c.quot_sw[i].p == quotient(c.quot_sw[i].w, q), "quotients of sn, sw [%zu]", i);
        for (size_t j = 0; j < L; ++j) {
            const agx::shoup_pair& w = c.quot_mat[j * (K + 1) + i];      // w q_j D_i = 1
            CHECK(w.w < q && mulmod(mulmod(w.w, Q[j] % q, q), i < K ? prod_mod(B, i, q) : 1 % q, q) == 1 % q && w.p == quotient(w.w, q), "mat[%zu][%zu]", j, i);
        }
    }
}

// one coefficient as the kernel takes it: a [L + K + 1] reduced coefficient words under Q, B, m; the accumulators are handed over anywhere in [0, 2q)
static std::vector<uint64_t> kernel_word(const std::vector<uint64_t>& B, const std::vector<uint64_t>& Q, uint64_t m, const built& b, const std::vector<uint64_t>& a) {
    const size_t K = B.size(), L = Q.size();
    const agx::basis_image& c = b.img;
    // the scaled inverses: the last stage multiplies by the scaled n^-1 in the place of n^-1, so a word a n^-1 becomes a (n^-1 scale)
    std::vector<uint64_t> y(L), s(K + 1), z(K, 0), out(L);
    for (size_t j = 0; j < L; ++j) y[j] = agx::bfv_shoup(mulmod(a[j], invmod(b.dn[j], Q[j]), Q[j]), c.quot_dn[j].w, c.quot_dn[j].p, Q[j]);
    for (size_t i = 0; i <= K; ++i) {
        const uint64_t q = i < K ? B[i] : m;
        s[i] = agx::bfv_shoup(mulmod(a[L + i], invmod(i < K ? b.sn[i] : b.an, q), q), c.quot_sn[i].w, c.quot_sn[i].p, q);
    }
    uint64_t fm = 0, wm = 0;
    for (size_t j = 0; j < L; ++j) {
        const agx::shoup_pair* row = &c.quot_mat[j * (K + 1)];
        for (size_t i = 0; i < K; ++i) z[i] = agx::quot_accumulate(z[i], y[j], row[i].w, row[i].p, B[i], B[i] << 1);
        fm = agx::quot_accumulate(fm, y[j], row[K].w, row[K].p, m, m << 1);
    }
    for (size_t i = 0; i < K; ++i) {
        z[i] = agx::quot_residue(s[i], z[i], B[i]);
        wm = agx::quot_accumulate(wm, z[i], c.aux_row[i].w, c.aux_row[i].p, m, m << 1);
    }
    fm = agx::quot_residue(s[K], fm, m);
    bool negative = false;
    const uint64_t mag = agx::bfv_centre(agx::bfv_alpha(wm >= m ? wm - m : wm, fm, c.k_exact.w, c.k_exact.p, m), m, &negative);
    for (size_t j = 0; j < L; ++j) {
        uint64_t acc = 0;
        for (size_t i = 0; i < K; ++i) acc = agx::quot_accumulate(acc, z[i], c.mat[j * K + i].w, c.mat[j * K + i].p, Q[j], Q[j] << 1);
        out[j] = agx::bfv_correct(acc, mag, negative, c.aux_corr_exact[j].w, c.aux_corr_exact[j].p, Q[j]);
    }
    return out;
}

// the contract's formula in modular arithmetic of its own; *alpha_out: the alpha it found, as a residue of m
static std::vector<uint64_t> contract_word(const std::vector<uint64_t>& B, const std::vector<uint64_t>& Q, uint64_t m, uint64_t t, const std::vector<uint64_t>& a,
                                           uint64_t* alpha_out) {
    const size_t K = B.size(), L = Q.size();
    std::vector<uint64_t> y(L), z(K), out(L);
    for (size_t j = 0; j < L; ++j) y[j] = mulmod(mulmod(t % Q[j], a[j], Q[j]), invmod(prod_mod(Q, j, Q[j]), Q[j]), Q[j]);
    auto v_mod = [&](uint64_t p) {
        u128 v = 0;
        for (size_t j = 0; j < L; ++j) v = (v + (u128)(y[j] % p) * prod_mod(Q, j, p)) % p;
        return (uint64_t)v;
    };
    auto floor_mod = [&](uint64_t p, uint64_t ap) { return mulmod(submod(mulmod(t % p, ap, p), v_mod(p), p), invmod(prod_mod(Q, L, p), p), p); };
    for (size_t i = 0; i < K; ++i) z[i] = mulmod(floor_mod(B[i], a[L + i]), invmod(prod_mod(B, i, B[i]), B[i]), B[i]);
    auto w_mod = [&](uint64_t p) {
        u128 w = 0;
        for (size_t i = 0; i < K; ++i) w = (w + (u128)(z[i] % p) * prod_mod(B, i, p)) % p;
        return (uint64_t)w;
    };
    const uint64_t alpha = mulmod(submod(w_mod(m), floor_mod(m, a[L + K]), m), invmod(prod_mod(B, K, m), m), m);
    *alpha_out = alpha;
    const bool negative = alpha > (m >> 1);
    const uint64_t mag = negative ? m - alpha : alpha;
    for (size_t j = 0; j < L; ++j) {
        const uint64_t q = Q[j], ab = mulmod(mag % q, prod_mod(B, K, q), q);
        out[j] = negative ? (uint64_t)(((u128)w_mod(q) + ab) % q) : submod(w_mod(q), ab, q);
    }
    return out;
}

static void check_words(const std::vector<uint64_t>& B, const std::vector<uint64_t>& Q, uint64_t m, uint64_t t, const built& b, int values) {
    const size_t K = B.size(), L = Q.size();
    const uint64_t half = m >> 1;
    const uint64_t edges[] = {half, half + 1, 0, 1 % m, m - 1};      // alpha = (m - 1) / 2, -(m - 1) / 2, 0, 1, -1
    for (int k = 0; k < values; ++k) {
        std::vector<uint64_t> a(L + K + 1);
        for (size_t j = 0; j < L; ++j) a[j] = k == 0 ? 0 : k == 1 ? Q[j] - 1 : next64() % Q[j];
        for (size_t i = 0; i < K; ++i) a[L + i] = k == 0 ? 0 : k == 1 ? B[i] - 1 : next64() % B[i];
        a[L + K] = next64() % m;
        uint64_t alpha = 0;
        if (k < 5 + 2 && k >= 2 && t % m) {
            // choose the auxiliary word for a wanted alpha: alpha is affine in a_m with slope -t D^-1 B^-1
            const uint64_t want = edges[k - 2];
            (void)contract_word(B, Q, m, t, a, &alpha);
            const uint64_t slope = mulmod(mulmod(t % m, invmod(prod_mod(Q, L, m), m), m), invmod(prod_mod(B, K, m), m), m);
            a[L + K] = (uint64_t)(((u128)a[L + K] + mulmod(submod(alpha, want, m), invmod(slope, m), m)) % m);
            const std::vector<uint64_t> w = contract_word(B, Q, m, t, a, &alpha);
            CHECK(alpha == want, "K=%zu L=%zu m=%llu: the wanted alpha was not reached", K, L, (ull)m);
            (void)w;
        }
        const std::vector<uint64_t> want = contract_word(B, Q, m, t, a, &alpha), got = kernel_word(B, Q, m, b, a);
        for (size_t j = 0; j < L; ++j)
            CHECK(got[j] == want[j] && got[j] < Q[j], "K=%zu L=%zu m=%llu t=%llu alpha=%llu: target %zu: %llu, not %llu", K, L, (ull)m, (ull)t, (ull)alpha, j, (ull)got[j], (ull)want[j]);
    }
}

int main(int argc, char** argv) {
    g_rng = 0x13198A2E03707344ull;
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
    selftest_section("bfv_quotient_arith");
    const size_t shapes[][2] = {{1, 1}, {1, 16}, {2, 3}, {16, 3}, {2, 1}, {16, 1}};      // {K, L}: K + L + 1 <= 20
    const uint64_t ts[] = {1, 2, 65537, ~(uint64_t)0 - 58};
    for (const auto& shape : shapes)
        for (size_t first = 0; first < M; ++first) {
            const size_t K = shape[0], L = shape[1];
            std::vector<uint64_t> B, Q;
            for (size_t k = 0; k < K; ++k) B.push_back(moduli[(first + k) % M]);
            const uint64_t m = moduli[(first + K) % M];
            for (size_t k = 0; k < L; ++k) Q.push_back(moduli[(first + K + 1 + k) % M]);
            const uint64_t t = ts[(first + K) % 4];
            const built b = build(B, Q, m, t);
            CHECK(b.fault == agx::basis_fault::none, "K=%zu L=%zu m=%llu: refused", K, L, (ull)m);
            if (b.fault != agx::basis_fault::none) continue;
            check_constants(B, Q, m, t, b);
            check_words(B, Q, m, t, b, 12);
            const built plain = build(B, Q, m, 0);
            CHECK(plain.fault == agx::basis_fault::none && plain.img.quot_mat.empty() && plain.img.quot_dn.empty() && plain.img.quot_sn.empty(), "constants without a t");
            std::vector<uint64_t> bad = Q;
            bad[L - 1] = B[0];
            CHECK(build(B, bad, m, t).fault == agx::basis_fault::quotient, "a target that is a source was accepted");
            if (L >= 2) {
                bad = Q, bad[0] = Q[L - 1];
                CHECK(build(B, bad, m, t).fault == agx::basis_fault::quotient, "two equal targets were accepted");
            }
        }
    std::printf("moduli: %zu\n", M);
    return selftest_report("bfv_quotient");
}
