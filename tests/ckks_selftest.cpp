// ckks_selftest.cpp -- csrc/ckks_arith.hpp (the text the CKKS kernels compile) and the tables of agx::prepare_ckks_image / agx::ckks_twiddle
// (csrc/host_math.cpp) against brute force in unsigned __int128.  Stand-alone: built by tests/test_ckks_selftest.py from this file and host_math.cpp only,
// under AddressSanitizer and UndefinedBehaviorSanitizer.  Arguments: the moduli (odd, > 1, < 2^62, distinct).  Prints its counts and "ok: N failures".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../agilex-ntt_amd/csrc/ckks_arith.hpp"
#include "../agilex-ntt_amd/csrc/host_math.hpp"

typedef unsigned __int128 u128;
typedef __int128 i128;
using namespace agx;

static long failures = 0;
static void fail(const char* what, double x, uint64_t q, uint64_t got, uint64_t want) {
    if (failures++ < 10) std::printf("FAIL %s: x = %a q = %llu got %llu want %llu\n", what, x, (unsigned long long)q, (unsigned long long)got, (unsigned long long)want);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// rint(x) mod q without rint: floor and the tie rule by hand below 2^63, the significand doubled e times from there on
static uint64_t brute_residue(double x, uint64_t q) {
    if (!std::isfinite(x)) return 0;
    const bool negative = std::signbit(x);
    const double a = std::fabs(x);
    uint64_t r;
    if (a < 9223372036854775808.0) {
        const double f = std::floor(a), frac = a - f;      // exact
        uint64_t c = (uint64_t)f;
        if (frac > 0.5 || (frac == 0.5 && (c & 1))) ++c;
        r = c % q;
    } else {
        int e;
        const double m = std::frexp(a, &e);      // a = m 2^e, m in [0.5, 1)
        u128 v = (u128)(uint64_t)std::ldexp(m, 53) % q;
        for (int k = 0; k < e - 53; ++k) v = v * 2 % q;
        r = (uint64_t)v;
    }
    return negative && r ? q - r : r;
}

static long check_round(const std::vector<uint64_t>& moduli) {
    ckks_image img;
    if (!prepare_ckks_image(img, moduli.data(), (uint32_t)moduli.size() > 16 ? 16 : (uint32_t)moduli.size(), 8)) { ++failures; return 0; }
    long checks = 0;
    std::vector<double> xs = {0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, 0.49999999999999994, 0.5000000000000001, 4503599627370495.5, 4503599627370496.5,
                              -4503599627370497.5, 9007199254740991.0, 9007199254740992.0, 9223372036854774784.0, 9223372036854775808.0, -9223372036854775808.0,
                              18446744073709551616.0, 4.9e-324, -4.9e-324, 2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308,
                              std::ldexp(1.0, 1000), -std::ldexp(1.0, 1000), std::ldexp(0x1.fffffffffffffp0, 1000), std::numeric_limits<double>::quiet_NaN(),
                              std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
    for (int e = -4; e <= 1000; e += 3)
        for (int k = 0; k < 6; ++k) {
            const double m = 1.0 + (double)(rnd() >> 11) * 0x1p-53;
            xs.push_back(std::ldexp(k & 1 ? -m : m, e));
            xs.push_back(std::ldexp((double)(rnd() % 1024) + 0.5, e > 40 ? 40 : e < 0 ? 0 : e));      // ties and near-ties at small exponents
        }
    const uint32_t L = (uint32_t)img.q.size();
    for (uint32_t i = 0; i < L; ++i)
        for (double x : xs) {
            bool negative;
            uint32_t e;
            const uint64_t mant = ckks_round(x, &negative, &e);
            if (e >= kCkksPow2) { fail("exponent", x, img.q[i], e, kCkksPow2); continue; }
            const shoup_pair& pw = img.pow2[(size_t)i * kCkksPow2 + e];
            const uint64_t got = ckks_residue(mant, negative, pw.w, pw.p, img.q[i]), want = brute_residue(x, img.q[i]);
            if (got != want) fail("residue", x, img.q[i], got, want);
            ++checks;
        }
    return checks;
}

// Horner over the digits a division gives: what the definition asks for, by another route to the digits
static double brute_double(i128 X, const uint64_t* q, uint32_t L) {
    const bool negative = X < 0;
    u128 mag = negative ? (u128)(-X) : (u128)X;
    std::vector<uint64_t> w(L);
    for (uint32_t i = 0; i < L; ++i) w[i] = (uint64_t)(mag % q[i]), mag /= q[i];
    double acc = (double)w[L - 1];
    for (int i = (int)L - 2; i >= 0; --i) {
        const double p = acc * (double)q[i];
        acc = p + (double)w[i];
    }
    return negative ? -acc : acc;
}

template <int SMAX>
static void check_value(i128 X, const uint64_t* q, uint32_t L, const ckks_image& img, long& checks) {
    uint64_t x[SMAX] = {};
    for (uint32_t i = 0; i < L; ++i) {
        const i128 r = X % (i128)q[i];
        x[i] = (uint64_t)(r < 0 ? r + (i128)q[i] : r);
    }
    const double got = ckks_rns_to_double<SMAX>(x, L, img.q.data(), reinterpret_cast<const uint64_t*>(img.tri.data())), want = brute_double(X, q, L);
    uint64_t gb, wb;
    std::memcpy(&gb, &got, 8), std::memcpy(&wb, &want, 8);
    if (gb != wb && !(got == 0.0 && want == 0.0)) fail("garner", want, q[0], gb, wb);
    ++checks;
}

template <int SMAX>
static void check_garner_set(const uint64_t* q, uint32_t L, long& checks) {
    ckks_image img;
    if (!prepare_ckks_image(img, q, L, 8)) { ++failures; return; }
    u128 D = 1;
    for (uint32_t i = 0; i < L; ++i) D *= q[i];
    const i128 half = (i128)((D - 1) / 2);
    std::vector<i128> xs = {0, 1, -1, half, -half, half - 1, -half + 1};
    u128 part = 1;
    for (uint32_t i = 0; i + 1 < L; ++i) {      // q_0 ... q_i: a carry through the digits below, and its neighbours
        part *= q[i];
        if ((i128)part <= half) xs.push_back((i128)part), xs.push_back(-(i128)part), xs.push_back(-(i128)part + 1), xs.push_back(-(i128)part - 1);
    }
    for (int k = 0; k < 400; ++k) {
        const u128 r = (((u128)rnd() << 64) | rnd()) % D;
        xs.push_back(r > (u128)half ? (i128)r - (i128)D : (i128)r);
    }
    for (i128 X : xs) check_value<SMAX>(X, q, L, img, checks);
}

static long check_garner(std::vector<uint64_t> moduli) {
    long checks = 0;
    for (size_t i = 0; i < moduli.size(); ++i) check_garner_set<1>(&moduli[i], 1, checks);
    for (size_t i = 0; i + 1 < moduli.size(); ++i) {      // two moduli, wide ones included: D < 2^124
        const uint64_t pair[2] = {moduli[i], moduli[i + 1]}, riap[2] = {moduli[i + 1], moduli[i]};
        check_garner_set<2>(pair, 2, checks), check_garner_set<2>(riap, 2, checks);
    }
    // the longest runs of the smallest moduli whose product stays below 2^126
    std::vector<uint64_t> asc = moduli;
    for (size_t i = 0; i < asc.size(); ++i)
        for (size_t j = i + 1; j < asc.size(); ++j)
            if (asc[j] < asc[i]) { const uint64_t t = asc[i]; asc[i] = asc[j], asc[j] = t; }
    u128 D = 1;
    uint32_t L = 0;
    while (L < asc.size() && L < 16 && D * asc[L] < ((u128)1 << 126) && D * asc[L] / asc[L] == D) D *= asc[L++];
    for (uint32_t l = 3; l <= L; ++l) {
        if (l <= 4) check_garner_set<4>(asc.data(), l, checks);
        else if (l <= 8) check_garner_set<8>(asc.data(), l, checks);
        else check_garner_set<16>(asc.data(), l, checks);
    }
    std::printf("garner: up to %u moduli against 128-bit brute force\n", L);
    // sixteen moduli, wide ones included: the values whose doubles are known without wide arithmetic
    if (moduli.size() >= 16) {
        ckks_image img;
        if (!prepare_ckks_image(img, moduli.data(), 16, 8)) { ++failures; return checks; }
        for (int v = -3; v <= 3; ++v) {
            uint64_t x[16];
            for (int i = 0; i < 16; ++i) {
                const int64_t q = (int64_t)moduli[i];
                x[i] = (uint64_t)((v % q + q) % q);
            }
            const double got = ckks_rns_to_double<16>(x, 16, img.q.data(), reinterpret_cast<const uint64_t*>(img.tri.data()));
            if (got != (double)v) fail("garner16", (double)v, moduli[0], (uint64_t)(int64_t)got, (uint64_t)(int64_t)v);
            ++checks;
        }
    }
    return checks;
}

static long check_twiddles() {
    long checks = 0;
    const long double pi = 3.141592653589793238462643383279502884L;
    double out[2] = {7, 7};
    if (ckks_twiddle(1, 0, out) || ckks_twiddle(3, 0, out) || ckks_twiddle(32768, 0, out) || ckks_twiddle(8, 4, out) || out[0] != 7 || out[1] != 7) ++failures;
    for (uint32_t len = 2; len <= 16384; len <<= 1) {
        uint64_t r = 1;
        for (uint32_t j = 0; j < len / 2; ++j, r = r * 5 % (4 * len)) {
            if (!ckks_twiddle(len, j, out)) { ++failures; continue; }
            const long double theta = 2.0L * pi * (long double)r / (long double)(4 * len);      // unreduced: a few 2^-64 worse than the table's route
            const long double dc = fabsl((long double)out[0] - cosl(theta)), ds = fabsl((long double)out[1] - sinl(theta));
            if (dc > 0x1p-53L + 0x1p-60L || ds > 0x1p-53L + 0x1p-60L) fail("twiddle", out[0], len, j, 0);
            ++checks;
        }
    }
    return checks;
}

int main(int argc, char** argv) {
    std::vector<uint64_t> moduli;
    for (int i = 1; i < argc; ++i) moduli.push_back(std::strtoull(argv[i], nullptr, 10));
    if (moduli.size() < 2) { std::printf("usage: ckks_selftest q0 q1 ...\n"); return 2; }
    std::printf("moduli: %zu\n", moduli.size());
    std::printf("ckks_round: %ld checks\n", check_round(moduli));
    std::printf("ckks_garner: %ld checks\n", check_garner(moduli));
    std::printf("ckks_twiddle: %ld checks\n", check_twiddles());
    // the butterflies: four products and two sums, nothing fused
    ckks_cplx a = {0x1.23456789abcdep0, -0x1.fedcba9876543p-1}, b = {0x1.0f0f0f0f0f0f1p-2, 0x1.7777777777777p1};
    const ckks_cplx tw = {0x1.6a09e667f3bcdp-1, 0x1.6a09e667f3bccp-1};
    const double rr = b.re * tw.re, ii = b.im * tw.im, ri = b.re * tw.im, ir = b.im * tw.re;
    const double wr = rr - ii, wi = ri + ir, er = a.re + wr, ei = a.im + wi, fr = a.re - wr, fi = a.im - wi;
    ckks_bfly_fwd(a, b, tw);
    if (a.re != er || a.im != ei || b.re != fr || b.im != fi) ++failures, std::printf("FAIL butterfly\n");
    std::printf("ok: %ld failures\n", failures);
    return failures ? 1 : 0;
}
