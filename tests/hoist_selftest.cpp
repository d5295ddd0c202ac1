// hoist_selftest.cpp -- the host-compilable parts of agx_ntt_keyswitch_decompose / _apply_decomposed and agx_ntt_inner_product_galois, by brute force.
// Stand-alone: built from this file, tests/selftest.hpp and csrc/keyswitch_layout.hpp alone by tests/test_selftests.py with -fsanitize=address,undefined; no HIP.
//   (a) csrc/keyswitch_layout.hpp: the three buffers of the two halves are the ext, coeff and acc parts of keyswitch_scratch_partition; counts past
//       2^60 words are reported and not wrapped; the launch counts of the two halves sum to keyswitch_launches.
//   (b) a host restatement of pi_g(i) = brev((g brev(i) + (g - 1) / 2) mod n), in the kernels' own 32-bit operations: it is a bijection,
//       pi_g(2i + 1) = pi_g(2i) XOR 1 (what the 16-byte form rests on), and an aligned block of 2^m outputs reads an aligned block of 2^m inputs.
//       Coverage: every odd g < 2n at every position for n = 2 ... 1024; for n = 2048 ... 32768 SAMPLED, to keep the run short under the sanitizers:
//       some 65 elements per size (the ends included) at every position for all three properties, and the pair property at every odd g < 2n on 512
//       positions per g.  For n = 2, 8, 64 and every g it is sigma_g on the evaluation points: position i holds the value at psi^(2 brev(i) + 1).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../agilex-ntt_amd/csrc/keyswitch_layout.hpp"
#include "selftest.hpp"

static void test_layout() {
    using agx::keyswitch_shape;
    for (const keyswitch_shape& k : {keyswitch_shape{4, 4, 2, 2}, keyswitch_shape{3, 4, 2, 2}, keyswitch_shape{4, 5, 1, 1}, keyswitch_shape{4, 4, 2, 4}, keyswitch_shape{7, 9, 3, 3}})
        for (uint32_t n : {2u, 64u, 4096u, 32768u})
            for (uint64_t batch : {(uint64_t)0, (uint64_t)1, (uint64_t)5, (uint64_t)4096}) {
                agx::keyswitch_scratch p;
                agx::keyswitch_hoisted h;
                CHECK(agx::keyswitch_scratch_partition(k, n, batch, &p) && agx::keyswitch_hoisted_partition(k, n, batch, &h), "a small partition refused");
                CHECK(h.decompose_scratch == p.ext - p.coeff && h.ext == p.acc - p.ext && h.apply_scratch == p.total - p.acc, "not the parts of the one scratch");
                CHECK(h.ext == (uint64_t)k.digits() * k.active() * batch * n && h.decompose_scratch == (uint64_t)k.q_count * batch * n &&
                          h.apply_scratch == 2ull * k.active() * batch * n, "not the documented sizes");
            }
    {
        agx::keyswitch_hoisted h;
        h.ext = h.decompose_scratch = h.apply_scratch = 77;
        const keyswitch_shape k{4, 4, 2, 2};      // ext and acc are 12 slabs each, coeff 4
        CHECK(!agx::keyswitch_hoisted_partition(k, 32768, (uint64_t)1 << 45, &h) && h.ext == 77 && h.decompose_scratch == 77 && h.apply_scratch == 77, "2^60 words per slab");
        CHECK(!agx::keyswitch_hoisted_partition(k, 4096, ~(uint64_t)0, &h) && h.ext == 77, "the largest batch");
        CHECK(!agx::keyswitch_hoisted_partition(k, 2, (uint64_t)1 << 63, &h), "batch n = 2^64 would wrap 64 bits to zero");
        CHECK(!agx::keyswitch_hoisted_partition(k, 32768, (uint64_t)1 << 49, &h), "batch n = 2^64");
        CHECK(!agx::keyswitch_hoisted_partition(k, 32768, (uint64_t)1 << 42, &h), "12 slabs of 2^57 words");
        // no call takes the three in one buffer: each is limited alone, where the one scratch (28 slabs of 2^56 words) is past the limit
        agx::keyswitch_scratch p;
        CHECK(agx::keyswitch_hoisted_partition(k, 32768, (uint64_t)1 << 41, &h) && h.ext == 12ull << 56 && h.decompose_scratch == 4ull << 56 && h.apply_scratch == 12ull << 56,
              "12 slabs of 2^56 words");
        CHECK(!agx::keyswitch_scratch_partition(k, 32768, (uint64_t)1 << 41, &p), "the one scratch at that size");
        const keyswitch_shape wide{256, 256, 16, 16};      // ext: 16 272 = 4352 slabs
        CHECK(agx::keyswitch_hoisted_partition(wide, 2, (uint64_t)1 << 46, &h) && h.ext == 4352ull << 47, "4352 slabs of 2^47 words");
        CHECK(!agx::keyswitch_hoisted_partition(wide, 2, (uint64_t)1 << 47, &h), "4352 slabs of 2^48 words");
    }
    {
        const int one[] = {1, 1}, pairs[] = {2, 2, 2, 2};
        CHECK(agx::keyswitch_launches_decompose(1, one, 2) == 3 && agx::keyswitch_launches_apply_decomposed(2) == 5, "two digits, fused routes");
        CHECK(agx::keyswitch_launches_decompose(2, pairs, 4) == 10 && agx::keyswitch_launches_apply_decomposed(7) == 15, "two digits apart, radix-2 at n = 32768");
        for (int inverse = 1; inverse <= 2; ++inverse)
            for (uint32_t calls = 0; calls <= 4; ++calls)
                for (int down = 2; down <= 7; ++down)
                    CHECK(agx::keyswitch_launches_decompose(inverse, pairs, calls) + agx::keyswitch_launches_apply_decomposed(down) == agx::keyswitch_launches(inverse, pairs, calls, down),
                          "the halves do not sum to the one call");
    }
}

// bit reversal of the low log_n bits, as the kernels form it: the 32-bit reversal shifted down
static uint32_t brev32(uint32_t x) {
    x = (x >> 16) | (x << 16);
    x = ((x & 0xff00ff00u) >> 8) | ((x & 0x00ff00ffu) << 8);
    x = ((x & 0xf0f0f0f0u) >> 4) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x & 0xccccccccu) >> 2) | ((x & 0x33333333u) << 2);
    return ((x & 0xaaaaaaaau) >> 1) | ((x & 0x55555555u) << 1);
}

// pi_g(p) in the kernel's operations (galois_read_index of csrc/inner_kernels.hpp, automorphism_ntt_kernel)
static uint32_t pi(uint32_t log_n, uint32_t g, uint32_t p) {
    const uint32_t mask = (1u << log_n) - 1u, shift = 32u - log_n, c = (g - 1u) >> 1;
    return brev32((g * (brev32(p) >> shift) + c) & mask) >> shift;
}

static void test_pi_structure() {
    for (uint32_t log_n = 1; log_n <= 15; ++log_n) {
        const uint32_t n = 1u << log_n;
        // every odd g up to n = 1024, a spread of 64 beyond (with the ends), so that the run stays short under the sanitizers
        const uint32_t step = n <= 1024 ? 2 : 2 * (n / 64) + 2;
        std::vector<uint32_t> image(n);
        std::vector<uint8_t> seen(n);
        std::vector<uint32_t> elements;
        for (uint32_t g = 1; g < 2 * n; g += step) elements.push_back(g);
        if (elements.back() != 2 * n - 1) elements.push_back(2 * n - 1);
        for (uint32_t g : elements) {
            std::fill(seen.begin(), seen.end(), 0);
            bool bijection = true, pairs = true, blocks = true;
            for (uint32_t i = 0; i < n; ++i) {
                image[i] = pi(log_n, g, i);
                if (image[i] >= n || seen[image[i]]++) bijection = false;
            }
            for (uint32_t i = 0; i < n; i += 2) pairs = pairs && image[i + 1] == (image[i] ^ 1u);
            for (uint32_t m = 1; m <= log_n; ++m)      // the 2^m outputs from an aligned start read one aligned block of 2^m inputs
                for (uint32_t i = 0; i < n; ++i) blocks = blocks && (image[i] >> m) == (image[i & ~((1u << m) - 1u)] >> m);
            CHECK(bijection, "n=%u g=%u: not a bijection", n, g);
            CHECK(pairs, "n=%u g=%u: pi(2i + 1) != pi(2i) ^ 1", n, g);
            CHECK(blocks, "n=%u g=%u: an aligned block of outputs reads more than one aligned block", n, g);
            if (g == 1)
                for (uint32_t i = 0; i < n; ++i) CHECK(image[i] == i, "n=%u: pi_1 is not the identity", n);
        }
    }
}

// the pair property for EVERY odd g < 2n and n = 2 ... 32768, from the one fact it rests on: pi(2i + 1) = pi(2i) ^ 1 iff the two k differ in the top
// bit only, and brev(2i + 1) = brev(2i) + n/2.  The full scan above covers n <= 1024; here every g at the larger sizes, on a spread of i.
static void test_pair_property_every_g() {
    for (uint32_t log_n = 11; log_n <= 15; ++log_n) {
        const uint32_t n = 1u << log_n;
        for (uint32_t g = 1; g < 2 * n; g += 2) {
            bool ok = true;
            for (uint32_t i = 0; i < n; i += n / 256) ok = ok && pi(log_n, g, i + 1) == (pi(log_n, g, i) ^ 1u) && pi(log_n, g, n - 1 - i) == (pi(log_n, g, n - 2 - i) ^ 1u);
            CHECK(ok, "n=%u g=%u: pi(2i + 1) != pi(2i) ^ 1", n, g);
        }
    }
}

static uint64_t pow_mod(uint64_t a, uint64_t e, uint64_t q) {
    uint64_t r = 1;
    for (; e; e >>= 1, a = mulmod(a, a, q))
        if (e & 1) r = mulmod(r, a, q);
    return r;
}

// pi_g is sigma_g on NTT-form frames: with position i holding a(psi^(2 brev(i) + 1)), (sigma_g a)(x) = a(x^g) at position i is a's word at pi_g(i)
static void test_pi_is_the_automorphism() {
    const uint64_t q = 65537;      // 2^16 + 1: 3 generates the whole group, so 3^(65536 / 2n) is a primitive 2n-th root of unity
    for (uint32_t log_n : {1u, 3u, 6u}) {
        const uint32_t n = 1u << log_n;
        const uint64_t psi = pow_mod(3, 65536 / (2 * n), q);
        std::vector<uint64_t> a(n);
        for (uint32_t k = 0; k < n; ++k) a[k] = (k * 2654435761u + 12345u) % q;
        auto at = [&](const std::vector<uint64_t>& poly, uint64_t x) {
            uint64_t r = 0;
            for (uint32_t k = n; k-- > 0;) r = (mulmod(r, x, q) + poly[k]) % q;
            return r;
        };
        auto ntt = [&](const std::vector<uint64_t>& poly) {
            std::vector<uint64_t> out(n);
            for (uint32_t i = 0; i < n; ++i) out[i] = at(poly, pow_mod(psi, 2 * (brev32(i) >> (32 - log_n)) + 1, q));
            return out;
        };
        const std::vector<uint64_t> ahat = ntt(a);
        for (uint32_t g = 1; g < 2 * n; g += 2) {
            std::vector<uint64_t> b(n, 0);      // a(X^g) mod X^n + 1
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t e = (uint32_t)((uint64_t)k * g % (2 * n));
                b[e % n] = e < n ? a[k] : (q - a[k]) % q;
            }
            const std::vector<uint64_t> bhat = ntt(b);
            bool same = true;
            for (uint32_t i = 0; i < n; ++i) same = same && bhat[i] == ahat[pi(log_n, g, i)];
            CHECK(same, "n=%u g=%u: pi_g is not sigma_g on the evaluation points", n, g);
        }
    }
}

int main() {
    test_layout();
    selftest_section("hoisted_layout");
    test_pi_structure();
    test_pair_property_every_g();
    test_pi_is_the_automorphism();
    return selftest_report("galois_pi");
}
