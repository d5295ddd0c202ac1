// batch_selftest.cpp -- csrc/batch_arith.hpp and plain_from_digits of csrc/plain_arith.hpp (the text the kernels compile; ckks_rns_to_double's own copy of the
// Garner and sign steps is pinned to the shared functions here), the index tables of
// agx::prepare_batch_image and the agx_ntt_plain_reduce constants of agx::prepare_plain_image (csrc/host_math.cpp) against brute force in unsigned __int128.
// Stand-alone: built by tests/test_batch_selftest.py from this file and host_math.cpp only, under AddressSanitizer and UndefinedBehaviorSanitizer.
// Arguments: the moduli (odd primes, < 2^62, distinct).  Prints its counts and "ok: N failures".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../agilex-ntt_amd/csrc/batch_arith.hpp"
#include "../agilex-ntt_amd/csrc/host_math.hpp"
#include "../agilex-ntt_amd/csrc/plain_arith.hpp"

typedef unsigned __int128 u128;
using namespace agx;

static long failures = 0;
static void fail(const char* what, uint64_t a, uint64_t b, uint64_t got, uint64_t want) {
    if (failures++ < 10)
        std::printf("FAIL %s: (%llu, %llu) got %llu want %llu\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)got, (unsigned long long)want);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((u128)a * b % q); }
static uint64_t powmod(uint64_t a, uint64_t e, uint64_t q) {
    uint64_t r = 1 % q;
    for (a %= q; e; e >>= 1, a = mulmod(a, a, q))
        if (e & 1) r = mulmod(r, a, q);
    return r;
}

// batch_reduce: any word modulo t, t any modulus in [2, 2^62)
static long check_reduce(const std::vector<uint64_t>& ts) {
    long checks = 0;
    for (uint64_t t : ts) {
        const uint64_t one_p = shoup_quotient(1, t);
        std::vector<uint64_t> zs = {0, 1, t - 1, t, t + 1, 2 * t - 1, 2 * t, 4 * t - 1, 4 * t, ~0ull, ~0ull - 1, 1ull << 63, (1ull << 63) - 1, ~0ull / t * t, ~0ull / t * t - 1};
        for (int k = 0; k < 400; ++k) zs.push_back(rnd() >> (k % 64));
        for (uint64_t z : zs) {
            const uint64_t got = batch_reduce(z, one_p, t);
            if (got != z % t) fail("batch_reduce", z, t, got, z % t);
            ++checks;
        }
    }
    return checks;
}

// batch_source: inside the frame of e whatever the table entry holds
static long check_source() {
    long checks = 0;
    for (uint32_t log_n = 1; log_n <= 15; ++log_n) {
        const uint64_t n = 1ull << log_n;
        for (int k = 0; k < 200; ++k) {
            const uint64_t frame = k < 4 ? (uint64_t)k : rnd() >> (8 + log_n), w = rnd() & (n - 1), e = frame * n + w;
            const uint32_t idx = k & 1 ? (uint32_t)rnd() : (uint32_t)(rnd() & (n - 1));
            const uint64_t got = batch_source(e, log_n, idx), want = frame * n + (idx & (n - 1));
            if (got != want || got / n != frame) fail("batch_source", e, idx, got, want);
            ++checks;
        }
    }
    return checks;
}

static uint32_t brev(uint32_t x, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) r = (r << 1) | ((x >> i) & 1u);
    return r;
}

// the tables of prepare_batch_image for the prime t at every size n with 2n | t - 1 up to 4096: permutations, inverse to each other, the exponents by repeated
// multiplication; psi primitive and (small t) the least by exhaustion; for n <= 64 the definition itself: the word at slot_to_word[j] of a transform in the
// library's order out[brev(k)] = m(psi^{2k+1}) is m(psi^{e_j})
static long check_tables(const std::vector<uint64_t>& ts) {
    long checks = 0;
    for (uint64_t t : ts)
        for (uint32_t n = 2; n <= 4096 && (t - 1) % (2ull * n) == 0; n <<= 1) {
            batch_image img;
            if (prepare_batch_image(img, n, t) != batch_fault::none) { fail("prepare_batch_image", n, t, 1, 0); continue; }
            const uint64_t M = 2ull * n;
            int lg = 0;
            while ((1u << lg) < n) ++lg;
            if (powmod(img.psi, n, t) != t - 1) fail("psi^n", n, t, powmod(img.psi, n, t), t - 1);
            if (t < 70000)
                for (uint64_t r = 2; r < img.psi; ++r)
                    if (powmod(r, n, t) == t - 1) { fail("least root", n, t, img.psi, r); break; }
            if (img.one_t.w != 1 || img.one_t.p != (uint64_t)(((u128)1 << 64) / t)) fail("one_t", n, t, img.one_t.p, 0);
            std::vector<uint64_t> exps(n);
            uint64_t e = 1;
            for (uint32_t j = 0; j < n / 2; ++j, e = e * 5 % M) exps[j] = e, exps[n / 2 + j] = M - e;
            std::vector<char> seen(n, 0);
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t w = img.slot_to_word[j];
                if (w >= n || seen[w]) { fail("permutation", n, j, w, 0); continue; }
                seen[w] = 1;
                if (w != brev((uint32_t)((exps[j] - 1) / 2), lg)) fail("pos", n, j, w, brev((uint32_t)((exps[j] - 1) / 2), lg));
                if (img.word_to_slot[w] != j) fail("inverse", n, j, img.word_to_slot[w], j);
                ++checks;
            }
            if (n > 64) continue;
            std::vector<uint64_t> m(n), out(n);
            for (auto& c : m) c = rnd() % t;
            auto eval = [&](uint64_t x) {
                uint64_t acc = 0;
                for (uint32_t i = n; i-- > 0;) acc = (mulmod(acc, x, t) + m[i]) % t;
                return acc;
            };
            for (uint32_t k = 0; k < n; ++k) out[brev(k, lg)] = eval(powmod(img.psi, 2 * k + 1, t));
            for (uint32_t j = 0; j < n; ++j) {
                const uint64_t want = eval(powmod(img.psi, exps[j], t));
                if (out[img.slot_to_word[j]] != want) fail("slot value", n, j, out[img.slot_to_word[j]], want);
                ++checks;
            }
        }
    return checks;
}

// The constants agx_ntt_plain_reduce adds to a plain_image, and ckks_garner_digits / ckks_digits_negative / plain_from_digits on them.  Inputs are built from
// chosen mixed-radix digits, so the expected value needs no integer wider than 128 bits: X mod D = sum v_i prod_{k<i} q_k, negative iff it exceeds (D - 1) / 2.
// For L <= 2 (D < 2^124) X itself is formed and centred in 128 bits as well, at 0, +-1, +-(D - 1) / 2 and random.
template <int SMAX>
static long check_digits(const std::vector<uint64_t>& q, uint64_t gamma, uint64_t t, long* skipped) {
    const uint32_t L = (uint32_t)q.size();
    std::vector<uint64_t> ones(L, 1);
    plain_image img;
    if (prepare_plain_image(img, plain_request{q.data(), L, ones.data(), ones.data(), gamma, t}) != plain_fault::none) { ++*skipped; return 0; }      // t shares a factor
    long checks = 0;
    if (img.q != q || img.radix_t.size() != L || img.tri.size() != (size_t)L * (L - 1) / 2) fail("image shape", L, t, img.radix_t.size(), L);
    uint64_t w = 1 % t;
    for (uint32_t i = 0; i < L; ++i, w = mulmod(w, q[i - 1] % t, t)) {      // the increment runs after the body: w = prod_{k < i} q_k mod t at entry i
        if (img.radix_t[i].w != w || img.radix_t[i].p != (uint64_t)(((u128)w << 64) / t)) fail("radix_t", i, t, img.radix_t[i].w, w);
        ++checks;
    }
    const uint64_t d_t = w;      // after the last increment: D mod t
    if (img.d_t.w != d_t) fail("d_t", L, t, img.d_t.w, d_t);
    for (uint32_t i = 1; i < L; ++i)
        for (uint32_t j = 0; j < i; ++j) {
            const shoup_pair c = img.tri[i * (i - 1) / 2 + j];
            if (mulmod(c.w, q[j] % q[i], q[i]) != 1 || c.p != (uint64_t)(((u128)c.w << 64) / q[i])) fail("tri", i, j, c.w, 0);
            ++checks;
        }
    const uint64_t* tri = reinterpret_cast<const uint64_t*>(img.tri.data());
    const uint64_t* row = reinterpret_cast<const uint64_t*>(img.radix_t.data());
    const uint64_t factors[] = {1, 0, t - 1, ~0ull, rnd()};
    for (int round = 0; round < 60; ++round) {
        uint64_t v[SMAX] = {}, x[SMAX] = {}, got_v[SMAX];
        for (uint32_t i = 0; i < L; ++i) {
            switch (round < 8 ? round : 8 + (int)(rnd() % 4)) {
                case 0: v[i] = 0; break;                                           // X = 0
                case 1: v[i] = i == 0; break;                                      // X = 1
                case 2: v[i] = q[i] - 1; break;                                    // X = -1
                case 3: v[i] = q[i] >> 1; break;                                   // X = (D - 1) / 2: the largest positive
                case 4: v[i] = (q[i] >> 1) + (i == 0); break;                      // X = -(D - 1) / 2: one above it
                case 5: v[i] = i == 0 ? (q[i] >> 1) - 1 : q[i] >> 1; break;        // one below
                case 6: v[i] = i + 1 == L ? q[i] >> 1 : rnd() % q[i]; break;       // the top digit ties: a lower one decides
                case 7: v[i] = i == 0 ? rnd() % q[i] : q[i] >> 1; break;           // only the lowest differs
                case 8: v[i] = rnd() % q[i]; break;
                case 9: v[i] = rnd() % 3 ? q[i] >> 1 : rnd() % q[i]; break;
                case 10: v[i] = q[i] - 1 - rnd() % 3; break;
                default: v[i] = rnd() % 3; break;
            }
        }
        for (uint32_t i = 0; i < L; ++i) {      // x_i = sum_k v_k prod_{j<k} q_j mod q_i
            uint64_t acc = 0, weight = 1 % q[i];
            for (uint32_t k = 0; k < L; ++k, weight = mulmod(weight, q[k - 1] % q[i], q[i])) acc = (acc + mulmod(v[k] % q[i], weight, q[i])) % q[i];
            x[i] = acc;
        }
        ckks_garner_digits<SMAX>(x, L, q.data(), tri, got_v);
        bool negative = false;
        for (uint32_t i = L; i-- > 0;) {
            if (got_v[i] != v[i]) fail("garner digit", i, q[i], got_v[i], v[i]);
            if (v[i] != q[i] >> 1) { negative = v[i] > q[i] >> 1; break; }
        }
        for (uint32_t i = 0; i < L; ++i)
            if (got_v[i] != v[i]) fail("garner digit", i, q[i], got_v[i], v[i]);
        if (L <= 2) {      // the sign from X itself
            const u128 D = L == 1 ? (u128)q[0] : (u128)q[0] * q[1], X = (u128)v[0] + (L == 2 ? (u128)v[1] * q[0] : 0);
            if ((X > (D - 1) / 2) != negative) fail("sign in 128 bits", L, t, negative, X > (D - 1) / 2);
        }
        const bool got_neg = ckks_digits_negative<SMAX>(got_v, L, q.data());
        if (got_neg != negative) fail("sign", L, t, got_neg, negative);
        {   // ckks_rns_to_double keeps steps (1) and (2) in its own body: the same residues must give it these digits and this sign -- steps (3) to (5) of
            // ckks_arith.hpp on the two functions' results, bit for bit
            uint64_t w[SMAX];
            bool carry = got_neg;
            for (uint32_t i = 0; i < L; ++i) {
                w[i] = got_v[i];
                if (got_neg) {
                    w[i] = q[i] - 1 - got_v[i];
                    if (carry) {
                        if (++w[i] == q[i]) w[i] = 0;
                        else carry = false;
                    }
                }
            }
            double acc = 0.0;
            for (uint32_t i = L; i-- > 0;) {
                const double p = acc * (double)q[i];
                acc = p + (double)w[i];
            }
            const double want = got_neg ? -acc : acc, got = ckks_rns_to_double<SMAX>(x, L, q.data(), tri);
            if (__builtin_memcmp(&got, &want, 8) != 0) fail("ckks_rns_to_double against the shared steps", L, round, (uint64_t)got, (uint64_t)want);
            ++checks;
        }
        uint64_t base = 0, weight = 1 % t;
        for (uint32_t i = 0; i < L; ++i, weight = mulmod(weight, q[i - 1] % t, t)) base = (uint64_t)(((u128)base + mulmod(v[i] % t, weight, t)) % t);
        if (negative) base = (base + t - d_t % t) % t;
        for (uint64_t factor : factors) {
            const uint64_t f = factor % t, got = plain_from_digits<SMAX>(got_v, got_neg, L, row, t, img.d_t.w, f, shoup_quotient(f, t)), want = mulmod(base, f, t);
            if (got != want || got >= t) fail("plain_from_digits", L, t, got, want);
            ++checks;
        }
    }
    return checks;
}

int main(int argc, char** argv) {
    std::vector<uint64_t> moduli;
    for (int i = 1; i < argc; ++i) moduli.push_back(std::strtoull(argv[i], nullptr, 10));
    if (moduli.size() < 17) { std::printf("need at least 17 moduli\n"); return 2; }
    std::printf("moduli: %zu\n", moduli.size());
    std::vector<uint64_t> ts = moduli;
    for (uint64_t t : {2ull, 3ull, 4ull, 1ull << 16, 1ull << 61, (1ull << 62) - 1, (1ull << 62) - 2, 65536ull * 3}) ts.push_back(t);
    std::printf("batch_reduce: %ld checks\n", check_reduce(ts));
    std::printf("batch_source: %ld checks\n", check_source());
    std::printf("batch_tables: %ld checks\n", check_tables(moduli));
    batch_image img;
    if (prepare_batch_image(img, 64, 129) != batch_fault::modulus || prepare_batch_image(img, 64, 193) != batch_fault::modulus ||
        prepare_batch_image(img, 2, (1ull << 62) + 1) != batch_fault::modulus || prepare_batch_image(img, 64, 257) != batch_fault::none)
        fail("prepare_batch_image faults", 0, 0, 0, 0);
    long digits = 0, skipped = 0;
    const uint64_t gamma = moduli.back();
    const std::vector<uint64_t> plain_ts = {2, 3, 4, 1ull << 16, 257, 65537, 65536ull * 3, (1ull << 61) - 1, 1ull << 61, (1ull << 62) - 2, (1ull << 62) - 1};
    for (uint32_t L = 1; L <= 16; ++L)
        for (uint32_t first : {0u, (uint32_t)moduli.size() - 1 - L}) {
            const std::vector<uint64_t> q(moduli.begin() + first, moduli.begin() + first + L);
            for (uint64_t t : plain_ts)
                digits += L <= 1 ? check_digits<1>(q, gamma, t, &skipped) : L <= 2 ? check_digits<2>(q, gamma, t, &skipped) : L <= 4 ? check_digits<4>(q, gamma, t, &skipped)
                        : L <= 8 ? check_digits<8>(q, gamma, t, &skipped) : check_digits<16>(q, gamma, t, &skipped);
        }
    std::printf("plain_digits: %ld checks, %ld (Q, t) pairs refused by the image\n", digits, skipped);
    std::printf("ok: %ld failures\n", failures);
    return failures ? 1 : 0;
}
