// moddown_modes_selftest.cpp -- the host side of agx_ntt_basis_mod_down_mode and agx_ntt_basis_create_plain against brute force: csrc/moddown_arith.hpp,
// the two per-word steps of AGX_RESCALE_ROUND and the very text the kernels compile, and agx::half_product_mod / agx::prepare_basis_image
// (csrc/host_math.cpp).  Stand-alone: built from this file, tests/selftest.hpp, moddown_arith.hpp, inner_reduce.hpp and host_math.cpp by
// tests/test_selftests.py with -fsanitize=address,undefined; no HIP, no plan.
//   Moduli: the arguments (the class edges of tests/modulus_cases.py: the primes next to 2^31, 2^60, 2^61 and 2^62, those next to 2^60 - 2^28, the
//   smallest admitted primes), at least 20 distinct odd primes.  S = 1, 2 and 16 sources taken from every position of the list, three targets behind them.
//   t = 1, 2, 65537, 2^64 - 59, and t = a source modulus and twice it, which must be refused.
//   * h mod q, h = floor(D / 2): D is formed as a multi-word integer here (up to 16 x 62 bits), halved, and reduced limb by limb in unsigned __int128;
//   * the scaled constants times t give the unscaled ones back; the matrix is t D_i mod q_j factor by factor in another order; c_i D_i = h (mod q_i);
//     hq_j = t h (mod q_j); every quotient is floor(w 2^64 / q); t = 1 leaves sn, sw and the matrix as they were;
//   * moddown_round_y gives (y + c) mod q_i in [0, q_i) at and next to the wrap, moddown_round_acc gives acc - hq (mod q_j) inside [0, 2q_j) and below
//     q_j where acc is;
//   * where t S D and 2048 D fit 126 bits, the whole ModDown through these constants and steps in exact integers: X - delta is divisible by D, delta = 0 (mod t),
//     the result is the quotient's residue, in both modes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../agilex-ntt_amd/csrc/host_math.hpp"
#include "../agilex-ntt_amd/csrc/moddown_arith.hpp"
#include "selftest.hpp"

typedef __int128 i128;
typedef unsigned long long ull;

// floor(prod src / 2) mod q through a multi-word product: little-endian 64-bit limbs, one factor at a time, then one shift and a Horner reduction
static uint64_t half_mod_brute(const std::vector<uint64_t>& src, uint64_t q) {
    std::vector<uint64_t> limbs = {1};
    for (uint64_t f : src) {
        uint64_t carry = 0;
        for (uint64_t& l : limbs) {
            const u128 v = (u128)l * f + carry;
            l = (uint64_t)v, carry = (uint64_t)(v >> 64);
        }
        if (carry) limbs.push_back(carry);
    }
    for (size_t k = 0; k < limbs.size(); ++k) limbs[k] = (limbs[k] >> 1) | (k + 1 < limbs.size() ? limbs[k + 1] << 63 : 0);
    u128 r = 0;
    for (size_t k = limbs.size(); k-- > 0;) r = ((r << 64) | limbs[k]) % q;
    return (uint64_t)r;
}

// D mod m (skip == S) or D_skip mod m, from the last factor to the first (the builder goes first to last)
static uint64_t d_mod_brute(const std::vector<uint64_t>& src, size_t skip, uint64_t m) {
    u128 r = 1 % m;
    for (size_t k = src.size(); k-- > 0;)
        if (k != skip) r = r * (u128)(src[k] % m) % m;
    return (uint64_t)r;
}

// a request without an m, its image, and the image of the same request with t = 1; ok: accepted, and every target has its D^-1
struct built {
    bool ok = false;
    std::vector<uint64_t> n_inv, w1n;
    agx::basis_image img, plain;
};

static built build(const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, uint32_t n, uint64_t t) {
    const size_t S = src.size(), T = dst.size();
    built b;
    b.n_inv.resize(S), b.w1n.resize(S);
    for (size_t i = 0; i < S; ++i) {
        CHECK(agx::inv_mod_euclid(n % src[i], src[i], &b.n_inv[i]), "n has no inverse modulo an odd prime");
        b.w1n[i] = next64() % src[i];
    }
    agx::basis_request rq{src.data(), (uint32_t)S, dst.data(), (uint32_t)T, b.n_inv.data(), b.w1n.data()};
    if (agx::prepare_basis_image(b.plain, rq) != agx::basis_fault::none || !b.plain.moddown_legal) return b;
    rq.t = t;
    b.ok = agx::prepare_basis_image(b.img, rq) == agx::basis_fault::none;
    if (b.ok) CHECK(b.img.sn.size() == S && b.img.sw.size() == S && b.img.round_src.size() == S && b.img.round_dst.size() == T && b.img.down_mat.size() == T * S, "sizes [S], [T], [T][S]");
    return b;
}

static void check_constants(const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, uint32_t n, uint64_t t) {
    const size_t S = src.size(), T = dst.size();
    const built b = build(src, dst, n, t);
    CHECK(b.ok, "S=%zu t=%llu: refused", S, (ull)t);
    if (!b.ok) return;
    for (size_t i = 0; i < S; ++i) {
        const uint64_t q = src[i], h = half_mod_brute(src, q);
        CHECK(agx::half_product_mod(src.data(), (uint32_t)S, q) == h, "S=%zu: h mod source %zu", S, i);
        CHECK(b.img.sn[i].w < q && b.img.sw[i].w < q && b.img.round_src[i].w < q, "S=%zu: constants of source %zu not reduced", S, i);
        CHECK(mulmod(b.img.sn[i].w, t % q, q) == b.plain.sn[i].w && mulmod(b.img.sw[i].w, t % q, q) == b.plain.sw[i].w, "S=%zu t=%llu: sn, sw of source %zu times t", S, (ull)t, i);
        CHECK(b.img.sn[i].p == (uint64_t)(((u128)b.img.sn[i].w << 64) / q) && b.img.sw[i].p == (uint64_t)(((u128)b.img.sw[i].w << 64) / q), "S=%zu: quotients of source %zu", S, i);
        CHECK(mulmod(b.img.round_src[i].w, d_mod_brute(src, i, q), q) == h, "S=%zu: c_%zu D_i != h", S, i);
        CHECK(b.plain.sn[i].w == mulmod(b.n_inv[i], b.img.dinv[i].w, q) && b.plain.sw[i].w == mulmod(b.w1n[i], b.img.dinv[i].w, q), "S=%zu: sn, sw of source %zu with t = 1", S, i);
        CHECK(b.img.round_src[i].p == q, "S=%zu: the second word of round_src[%zu] is not the modulus", S, i);
        if (t == 1) CHECK(b.img.sn[i].w == b.plain.sn[i].w && b.img.sw[i].w == b.plain.sw[i].w, "t = 1 changed sn or sw");
    }
    for (size_t j = 0; j < T; ++j) {
        const uint64_t q = dst[j], h = half_mod_brute(src, q);
        CHECK(agx::half_product_mod(src.data(), (uint32_t)S, q) == h, "S=%zu: h mod target %zu", S, j);
        CHECK(b.img.round_dst[j] == mulmod(t % q, h, q), "S=%zu t=%llu: hq[%zu]", S, (ull)t, j);
        for (size_t i = 0; i < S; ++i) {
            const size_t at = j * S + i;
            CHECK(b.img.down_mat[at].w == mulmod(t % q, d_mod_brute(src, i, q), q), "S=%zu t=%llu: matrix [%zu][%zu]", S, (ull)t, j, i);
            CHECK(b.img.down_mat[at].p == (uint64_t)(((u128)b.img.down_mat[at].w << 64) / q), "S=%zu: quotient of matrix [%zu][%zu]", S, j, i);
            if (t == 1) CHECK(b.img.down_mat[at].w == b.img.mat[at].w && b.img.down_mat[at].p == b.img.mat[at].p, "t = 1 changed the matrix");
        }
    }
}

static void check_refused(const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, uint32_t n) {
    for (size_t i = 0; i < src.size(); i += src.size() > 2 ? 5 : 1) {
        CHECK(!build(src, dst, n, src[i]).ok, "t = source %zu accepted", i);
        CHECK(!build(src, dst, n, 2 * src[i]).ok, "t = twice source %zu accepted", i);      // below 2^63
    }
    CHECK(build(src, dst, n, dst[0]).ok, "t = a target modulus refused");      // t need not be invertible there
}

static void check_steps(uint64_t q) {
    const uint64_t ys[] = {0, 1 % q, q / 2, q - 1, next64() % q, next64() % q};
    for (uint64_t c : ys)
        for (uint64_t y : ys)
            for (uint64_t yy : {y, (q - c) % q, (q - c + q - 1) % q, (q - c + 1) % q}) {      // at the wrap and on both sides of it
                const uint64_t got = agx::moddown_round_y(yy, c, q);
                CHECK(got == (uint64_t)(((u128)yy + c) % q) && got < q, "q=%llu: %llu + %llu gave %llu", (ull)q, (ull)yy, (ull)c, (ull)got);
            }
    const uint64_t accs[] = {0, 1 % q, q - 1, q, q + 1, 2 * q - 1, next64() % (2 * q), next64() % (2 * q)};
    for (uint64_t hq : ys)
        for (uint64_t acc : accs)
            for (uint64_t a : {acc, hq, hq ? hq - 1 : 0, hq + 1, hq + q}) {      // at hq (the turn), next to it, and the same one q higher
                if (a >= 2 * q) continue;
                const uint64_t got = agx::moddown_round_acc(a, hq, q);
                CHECK(got < 2 * q && got % q == (uint64_t)(((u128)a + q - hq) % q), "q=%llu: %llu - %llu gave %llu", (ull)q, (ull)a, (ull)hq, (ull)got);
                if (a < q) CHECK(got < q, "q=%llu: a reduced accumulator left [0, q)", (ull)q);
            }
}

static int bits_of(u128 v) {
    int b = 0;
    while (v) ++b, v >>= 1;
    return b;
}

// the whole ModDown through the constants and the per-word steps, against exact integers; needs t S D below 2^127
static void check_mod_down(const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, uint32_t n, uint64_t t, int values) {
    const size_t S = src.size(), T = dst.size();
    u128 D = 1;
    int dbits = 0;
    for (uint64_t q : src) dbits += bits_of(q);
    if (dbits + bits_of(t) + bits_of(S) > 126 || dbits + 11 > 126) return;      // delta = t (V - h) and X = D Y + r with Y <= 1000 both fit a signed 128-bit word
    for (uint64_t q : src) D *= q;
    const built b = build(src, dst, n, t);
    CHECK(b.ok, "refused");
    if (!b.ok) return;
    std::vector<u128> Di(S, 1);
    for (size_t i = 0; i < S; ++i)
        for (size_t k = 0; k < S; ++k)
            if (k != i) Di[i] *= src[k];
    const u128 H = D / 2;
    std::vector<u128> rs = {0, 1, H - 1, H, H + 1, D - 1};
    for (int k = 0; k < values; ++k) rs.push_back(next128() % D);
    for (int round = 0; round < 2; ++round) {
        const u128 h = round ? H : 0;
        for (const u128 r : rs) {
            const u128 Y = 1 + next64() % 1000, X = D * Y + r;
            u128 V = 0;
            std::vector<uint64_t> y(S);
            for (size_t i = 0; i < S; ++i) {
                const uint64_t q = src[i];
                y[i] = mulmod(mulmod((uint64_t)(r % q), n % q, q), b.img.sn[i].w, q);      // what the scaled inverse writes: p_i t^-1 D_i^-1
                if (round) y[i] = agx::moddown_round_y(y[i], b.img.round_src[i].w, q);
                V += (u128)y[i] * Di[i];
            }
            CHECK(V / D < S, "V is not below S D");
            const i128 delta = (i128)t * ((i128)V - (i128)h);
            CHECK(((i128)X - delta) % (i128)D == 0, "S=%zu t=%llu mode %d: X - delta is not divisible by D", S, (ull)t, round);
            CHECK(delta % (i128)t == 0, "delta is not 0 modulo t");
            const i128 quotient = ((i128)X - delta) / (i128)D;
            for (size_t j = 0; j < T; ++j) {
                const uint64_t q = dst[j];
                uint64_t acc = 0;
                for (size_t i = 0; i < S; ++i) acc = (acc + mulmod(y[i] % q, b.img.down_mat[j * S + i].w, q)) % (2 * q);      // in [0, 2q), as basis_accumulate leaves it
                if (round) acc = agx::moddown_round_acc(acc, b.img.round_dst[j], q);
                const uint64_t got = mulmod((uint64_t)((X % q + 2 * (u128)q - acc) % q), b.img.dall[j].w, q);
                const i128 m = quotient % (i128)q;
                CHECK(got == (uint64_t)(m < 0 ? m + (i128)q : m), "S=%zu t=%llu mode %d: target %zu", S, (ull)t, round, j);
            }
        }
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
    const uint32_t n = 8;      // every odd modulus has an n^-1; the transform size enters the constants through n^-1 alone
    const uint64_t ts[] = {1, 2, 65537, ~0ull - 58};      // 2^64 - 59
    for (uint64_t q : moduli) check_steps(q);
    selftest_section("moddown_arith");
    for (size_t S : {(size_t)1, (size_t)2, (size_t)16})
        for (size_t first = 0; first < M; ++first) {
            std::vector<uint64_t> src, dst;
            for (size_t k = 0; k < S; ++k) src.push_back(moduli[(first + k) % M]);
            for (size_t k = 0; k < 3; ++k) dst.push_back(moduli[(first + S + k) % M]);
            for (uint64_t t : ts) {
                bool zero = false;
                for (uint64_t q : src) zero |= t % q == 0;
                if (zero) {
                    CHECK(!build(src, dst, n, t).ok, "t = 0 modulo a source accepted");
                    continue;
                }
                check_constants(src, dst, n, t);
                check_mod_down(src, dst, n, t, 40);
            }
            check_refused(src, dst, n);
        }
    std::printf("moduli: %zu\n", M);
    return selftest_report("moddown_mode_constants");
}
