// fold_selftest.cpp -- agx::fold_twiddle_pack (csrc/host_math.cpp) and the arithmetic of the two-twiddle butterfly for q = 2^60 - c, 0 < c < 2^28
// (csrc/modarith.hpp: ct_butterfly_q60c_fold), against brute force in unsigned __int128.
// Stand-alone: built from this file, tests/selftest.hpp and host_math.cpp by tests/test_selftests.py with -fsanitize=address,undefined; no HIP, no plan.
//   * the packing: wC = w 2^32 mod q, low halves below 2^29, high halves below 2^31, w and wC recombine exactly from the packed words;
//     w in {0, 1, q-1, 2^29-1, 2^29} and random, for the four benchmark primes (the largest 60-bit primes = 1 mod 8192) and both boundary primes of
//     tests/golden/q60c_boundary.json;
//   * the butterfly restated in plain C++ (the sign-bit subtract, the six-link chain, y' = 2 tx + 8q - x'), every partial sum taken in 128 bits and
//     checked below 2^64, x' = x + w y and y' = x - w y (mod q), on the corners of the 64-bit range for x and y and the corner twiddles;
//   * the bounds of the whole class evaluated at c = 2^28 - 1 and c = 1 (q60c_fold_bounds states them at compile time for the device code).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../agilex-ntt_amd/csrc/host_math.hpp"
#include "selftest.hpp"

static const u128 kTwo64 = (u128)1 << 64;
static const uint64_t kTop = 1ull << 60, kLow29 = (1ull << 29) - 1;

struct halves {
    uint64_t wl, wh, cl, ch;
};
static halves unpack(const agx::fold_twiddle& f) { return {f.w_packed & 0xffffffffull, f.w_packed >> 32, f.wc_packed & 0xffffffffull, f.wc_packed >> 32}; }

static void check_packing(uint64_t w, uint64_t q) {
    const halves h = unpack(agx::fold_twiddle_pack(w, q));
    const uint64_t wc = (uint64_t)(((u128)w << 32) % q);
    CHECK(h.wl < (1ull << 29) && h.cl < (1ull << 29), "q=%llu w=%llu: a low half at or above 2^29", (unsigned long long)q, (unsigned long long)w);
    CHECK(h.wh < (1ull << 31) && h.ch < (1ull << 31), "q=%llu w=%llu: a high half at or above 2^31", (unsigned long long)q, (unsigned long long)w);
    CHECK((h.wl | h.wh << 29) == w && h.wl == (w & kLow29), "q=%llu w=%llu: w does not recombine", (unsigned long long)q, (unsigned long long)w);
    CHECK((h.cl | h.ch << 29) == wc && h.cl == (wc & kLow29), "q=%llu w=%llu: wC is not w 2^32 mod q", (unsigned long long)q, (unsigned long long)w);
}

// one butterfly as the device code runs it, every sum in 128 bits; subtract: every stage but the first
static void check_butterfly(uint64_t x, uint64_t y, uint64_t w, uint64_t q, bool subtract) {
    const uint64_t c = kTop - q;
    const halves h = unpack(agx::fold_twiddle_pack(w, q));
    const u128 y0 = y & 0xffffffffull, y1 = y >> 32;
    u128 tx = x;
    if (subtract) {
        tx = (u128)(x & 0x7fffffffffffffffull) + (u128)(x >> 63) * (8 * c);      // csub_8q_q60c
        CHECK(tx <= ((u128)1 << 63) + 8 * c - 1, "q=%llu x=%llu: tx past 2^63 + 8c - 1", (unsigned long long)q, (unsigned long long)x);
    }
    CHECK(tx % q == x % q, "q=%llu x=%llu: the subtract changed the residue", (unsigned long long)q, (unsigned long long)x);
    const u128 hi0 = y0 * h.wh, hi = hi0 + y1 * h.ch;
    CHECK(hi < kTwo64, "q=%llu y=%llu w=%llu: hi wraps", (unsigned long long)q, (unsigned long long)y, (unsigned long long)w);
    const u128 hl = hi & 0xffffffffull, hh = hi >> 32;
    const u128 s1 = tx + y0 * h.wl, s2 = s1 + y1 * h.cl, s3 = s2 + hl * ((u128)1 << 29), xn = s3 + hh * (2 * c);
    CHECK(s1 < kTwo64 && s2 < kTwo64 && s3 < kTwo64 && xn < kTwo64, "q=%llu x=%llu y=%llu w=%llu: a partial sum of the chain wraps", (unsigned long long)q,
          (unsigned long long)x, (unsigned long long)y, (unsigned long long)w);
    const u128 Q = xn - tx, q8 = (u128)8 * q;
    CHECK(Q <= q8, "q=%llu y=%llu w=%llu: Q above 8q", (unsigned long long)q, (unsigned long long)y, (unsigned long long)w);
    const u128 t2 = 2 * tx + q8;      // the device forms it mod 2^64 and subtracts x': only the difference has to fit
    const u128 yn = t2 - xn;
    CHECK(t2 >= xn && yn < kTwo64, "q=%llu x=%llu y=%llu w=%llu: y' outside [0, 2^64)", (unsigned long long)q, (unsigned long long)x, (unsigned long long)y,
          (unsigned long long)w);
    const uint64_t wy = (uint64_t)((u128)(y % q) * w % q), xr = x % q;
    CHECK((uint64_t)(xn % q) == (xr + wy) % q, "q=%llu x=%llu y=%llu w=%llu: x' is not x + w y", (unsigned long long)q, (unsigned long long)x, (unsigned long long)y,
          (unsigned long long)w);
    CHECK((uint64_t)(yn % q) == (xr + q - wy) % q, "q=%llu x=%llu y=%llu w=%llu: y' is not x - w y", (unsigned long long)q, (unsigned long long)x, (unsigned long long)y,
          (unsigned long long)w);
}

// the class-wide bounds at one value of c, with the extreme operands (not tied to a prime: pure inequalities)
static void check_class_bounds(uint64_t c) {
    const u128 q = kTop - c, w32 = 0xffffffffull;
    const u128 wh_max = (uint64_t)(q - 1) >> 29, wl_max = kLow29;
    const u128 hi_max = 2 * w32 * wh_max, lo_max = 2 * w32 * wl_max;
    const u128 Q_max = lo_max + w32 * ((u128)1 << 29) + w32 * 2 * c, tx_max = ((u128)1 << 63) + 8 * c - 1;
    CHECK(wh_max < ((u128)1 << 31), "c=%llu: a twiddle's high half does not fit 31 bits", (unsigned long long)c);
    CHECK(hi_max < kTwo64, "c=%llu: hi_max wraps", (unsigned long long)c);
    CHECK(tx_max + Q_max < kTwo64, "c=%llu: tx_max + Q_max wraps", (unsigned long long)c);
    CHECK(Q_max <= 8 * q, "c=%llu: Q_max above 8q", (unsigned long long)c);
    CHECK(tx_max + 8 * q == kTwo64 - 1, "c=%llu: tx_max + 8q is not 2^64 - 1", (unsigned long long)c);
    CHECK((((u128)1 << 61) - 2 * c) % q == 0, "c=%llu: 2^61 is not 2c mod q", (unsigned long long)c);
}

int main() {
    std::vector<uint64_t> primes = agx::find_ntt_primes(60, 4096, 4);      // the benchmark's moduli
    CHECK(primes.size() == 4, "four 60-bit primes expected");
    primes.push_back(1152921504606830593ull);      // tests/golden/q60c_boundary.json: the smallest and the largest c below 2^28
    primes.push_back(1152921504338821121ull);
    for (uint64_t q : primes) {
        const uint64_t c = kTop - q;
        CHECK(q < kTop && c > 0 && c < (1ull << 28) && q % 8192 == 1 && agx::is_prime_u64(q), "q=%llu is not of the class", (unsigned long long)q);
        std::vector<uint64_t> ws = {0, 1, q - 1, q - 2, kLow29, kLow29 + 1, 1ull << 59, (1ull << 32) % q, q >> 1};
        for (int i = 0; i < 3000; ++i) ws.push_back(next64() % q);
        for (uint64_t w : ws) check_packing(w, q);
        const uint64_t corners[] = {0, 1, q - 1, q, 4 * q - 1, 8 * q - 1, 8 * q, (1ull << 63) - 1, 1ull << 63, (1ull << 63) + 1, 0xffffffffull, 0xffffffff00000000ull,
                                    0xffffffffffffffffull, 0x7fffffffffffffffull + 8 * c};
        const uint64_t wcorners[] = {1, q - 1, q - 2, kLow29, kLow29 + 1, 1ull << 59, 0};
        for (uint64_t x : corners)
            for (uint64_t y : corners)
                for (uint64_t w : wcorners) {
                    check_butterfly(x, y, w, q, true);
                    if (x < 4 * q) check_butterfly(x, y, w, q, false);      // a first-stage x is below 4q; y may be anything for the arithmetic
                }
        for (int i = 0; i < 20000; ++i) {
            const uint64_t x = next64(), y = next64(), w = next64() % q;
            check_butterfly(x, y, w, q, true);
            check_butterfly(x % (4 * q), y % (4 * q), w, q, false);
            check_butterfly(corners[i % 14], y, wcorners[i % 7], q, true);
            check_butterfly(x, corners[i % 14], w, q, true);
        }
    }
    check_class_bounds((1ull << 28) - 1);
    check_class_bounds(1);
    check_class_bounds(16383);
    return selftest_report("fold_twiddle_pack / two-twiddle butterfly");
}
