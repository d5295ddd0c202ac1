// sample_selftest.cpp -- csrc/sample_arith.hpp, the per-cell and per-word steps of agx_ntt_sample_uniform / _ternary / _cbd and the very text the kernels compile,
// against the standard ChaCha20 vectors and a brute-force restatement.  Stand-alone: built from this file, tests/selftest.hpp and sample_arith.hpp by
// tests/test_sample_selftest.py with -fsanitize=address,undefined; no HIP, no plan.
//   Moduli: the arguments (the class edges of tests/modulus_cases.py and the smallest admitted primes), at least 20 distinct odd primes.
//   * vectors: the zero key with w12..15 = 0 (the keystream's first 32 bytes) and RFC 8439 section 2.3.2 (key = bytes 0..31; the first four and last two words);
//   * uniform: sample_uniform_cell with W = 2, 4 and 8 against a walk written here on a list (blocks in order, candidates in order, masked, kept while below q),
//     for every modulus and several cells; the blocks it asks for are consecutive from 0 and stop when the words are in;
//   * uniform cap: a block source that returns rejected candidates only gives zeros after block 15 and is never asked for block 16; one that accepts from
//     block 15 on still fills the cell;
//   * ternary: 0xFF..FF -> 0, ..FD -> +1, ..FE -> -1, the first field that is not 3 at r = 0, 15 and 31, random words against the loop over the fields;
//   * cbd: eta = 1, 21 and 32 (and every other) on 0, all ones, alternating halves and random words against a bit loop;
//   * residue: every v in [-32, 32] under every modulus.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../agilex-ntt_amd/csrc/sample_arith.hpp"
#include "selftest.hpp"

typedef unsigned long long ull;

static agx::sample_key key_of(const uint8_t bytes[32]) {
    agx::sample_key k;
    for (int i = 0; i < 8; ++i) k.w[i] = (uint32_t)bytes[4 * i] | (uint32_t)bytes[4 * i + 1] << 8 | (uint32_t)bytes[4 * i + 2] << 16 | (uint32_t)bytes[4 * i + 3] << 24;
    return k;
}

static void check_vectors() {
    uint8_t zero[32] = {0}, seq[32];
    for (int i = 0; i < 32; ++i) seq[i] = (uint8_t)i;
    uint32_t o[16];
    agx::sample_block(key_of(zero), 0, 0, 0, 0, o);
    const uint8_t want[32] = {0x76, 0xb8, 0xe0, 0xad, 0xa0, 0xf1, 0x3d, 0x90, 0x40, 0x5d, 0x6a, 0xe5, 0x53, 0x86, 0xbd, 0x28,
                              0xbd, 0xd2, 0x19, 0xb8, 0xa0, 0x8d, 0xed, 0x1a, 0xa8, 0x36, 0xef, 0xcc, 0x8b, 0x77, 0x0d, 0xc7};
    for (int i = 0; i < 32; ++i) CHECK((uint8_t)(o[i / 4] >> (8 * (i % 4))) == want[i], "zero key, byte %d", i);
    agx::sample_block(key_of(seq), 1, 0x09000000u, 0x4a000000u, 0, o);
    CHECK(o[0] == 0xe4e7f110u && o[1] == 0x15593bd1u && o[2] == 0x1fdd0f50u && o[3] == 0xc47120a3u, "RFC 8439 2.3.2: %08x %08x %08x %08x", o[0], o[1], o[2], o[3]);
    CHECK(o[14] == 0xe883d0cbu && o[15] == 0x4e3c50a2u, "RFC 8439 2.3.2: ... %08x %08x", o[14], o[15]);
    CHECK(agx::sample_candidate(o, 0) == (((uint64_t)0x15593bd1u << 32) | 0xe4e7f110u) && agx::sample_candidate(o, 7) == (((uint64_t)0x4e3c50a2u << 32) | 0xe883d0cbu));
    CHECK(agx::sample_w12(0xFFFF, 4095, 15) == 0xFFFFFFFFu && agx::sample_w12(3, 5, 2) == 0x00030052u);
}

static uint32_t bitlen(uint64_t q) {
    uint32_t b = 0;
    while (q) ++b, q >>= 1;
    return b;
}

static void check_uniform(uint64_t q, const agx::sample_key& key) {
    const uint32_t bits = bitlen(q);
    const uint64_t mask = bits == 64 ? ~(uint64_t)0 : ((uint64_t)1 << bits) - 1;
    CHECK(agx::sample_mask(q) == mask, "mask of %llu", (ull)q);
    for (uint32_t W : {2u, 4u, 8u})
        for (uint32_t cell = 0; cell < 24; ++cell) {
            const uint32_t w12 = agx::sample_w12((uint32_t)(q % 65535), cell, 0), w13 = (uint32_t)next64(), w14 = (uint32_t)next64(), w15 = (uint32_t)next64();
            std::vector<uint32_t> asked;
            uint64_t got[8];
            agx::sample_uniform_cell([&](uint32_t k, uint32_t o[16]) { asked.push_back(k), agx::sample_block(key, w12 | k, w13, w14, w15, o); }, q, mask, W, got);
            // the restatement: every candidate of blocks 0 .. 15 in order on one list, the first W below q
            std::vector<uint64_t> kept;
            uint32_t blocks = 0;
            for (uint32_t k = 0; k < 16 && kept.size() < W; ++k, ++blocks) {
                uint32_t o[16];
                agx::sample_block(key, w12 | k, w13, w14, w15, o);
                for (int i = 0; i < 8; ++i) {
                    const uint64_t v = (((uint64_t)o[2 * i + 1] << 32) | o[2 * i]) & mask;
                    if (v < q) kept.push_back(v);
                }
            }
            kept.resize(W, 0);
            for (uint32_t r = 0; r < 8; ++r) CHECK(got[r] == (r < W ? kept[r] : 0) && got[r] < q, "q=%llu W=%u cell %u word %u: %llu", (ull)q, W, cell, r, (ull)got[r]);
            CHECK(asked.size() == blocks, "q=%llu W=%u: %zu blocks asked, %u needed", (ull)q, W, asked.size(), blocks);
            for (size_t k = 0; k < asked.size(); ++k) CHECK(asked[k] == k);
        }
}

static void check_cap(uint64_t q) {
    const uint64_t mask = agx::sample_mask(q);
    if (mask == q) return;      // no candidate can be rejected (no admitted modulus is 2^b - 1, but an argument may be)
    for (uint32_t W : {2u, 4u, 8u}) {
        uint32_t asked = 0, highest = 0;
        uint64_t got[8];
        for (int r = 0; r < 8; ++r) got[r] = 0x5555;
        agx::sample_uniform_cell([&](uint32_t k, uint32_t o[16]) { ++asked, highest = k > highest ? k : highest; for (int i = 0; i < 16; ++i) o[i] = 0xffffffffu; }, q, mask, W, got);
        CHECK(asked == 16 && highest == 15, "q=%llu W=%u: %u blocks asked, the highest %u", (ull)q, W, asked, highest);
        for (int r = 0; r < 8; ++r) CHECK(got[r] == 0, "q=%llu W=%u word %d is %llu", (ull)q, W, r, (ull)got[r]);
        // accepted values 1, 2, ... from block 15 on only: the cell is filled while W <= 8 candidates are enough, and block 16 is never read
        asked = 0;
        uint32_t value = 0;
        agx::sample_uniform_cell([&](uint32_t k, uint32_t o[16]) {
            ++asked;
            CHECK(k < 16);
            for (int i = 0; i < 16; ++i) o[i] = k < 15 ? 0xffffffffu : (i & 1 ? 0u : (++value) % (uint32_t)(q < 5 ? q : 5));
        }, q, mask, W, got);
        CHECK(asked == 16);
        for (uint32_t r = 0; r < 8; ++r) CHECK(got[r] == (r < W ? (r + 1) % (q < 5 ? q : 5) : 0), "q=%llu W=%u late word %u is %llu", (ull)q, W, r, (ull)got[r]);
    }
}

static int ternary_loop(uint64_t w) {
    for (int r = 0; r < 32; ++r) {
        const unsigned f = (unsigned)(w >> (2 * r)) & 3u;
        if (f != 3) return f == 0 ? 0 : f == 1 ? 1 : -1;
    }
    return 0;
}

static void check_ternary() {
    const uint64_t ones = ~(uint64_t)0;
    CHECK(agx::sample_ternary(ones) == 0 && agx::sample_ternary(ones - 2) == 1 && agx::sample_ternary(ones - 1) == -1);
    for (int r : {0, 15, 31}) {
        const uint64_t low = r ? ((uint64_t)1 << (2 * r)) - 1 : 0;
        CHECK(agx::sample_ternary(low | (uint64_t)1 << (2 * r)) == 1 && agx::sample_ternary(low | (uint64_t)2 << (2 * r)) == -1 && agx::sample_ternary(low) == 0, "r = %d", r);
        const uint64_t high = r < 31 ? next64() << (2 * r + 2) : 0;      // fields above r do not matter
        CHECK(agx::sample_ternary(high | low | (uint64_t)2 << (2 * r)) == -1, "r = %d", r);
    }
    for (int it = 0; it < 20000; ++it) {
        uint64_t w = next64();
        if (it & 1) w |= ((uint64_t)1 << (2 * (it % 33) % 64)) - 1;      // runs of fields 3 in front
        CHECK(agx::sample_ternary(w) == ternary_loop(w), "word %llx", (ull)w);
    }
}

static int cbd_loop(uint64_t w, uint32_t eta) {
    int v = 0;
    for (uint32_t b = 0; b < eta; ++b) v += (int)((w >> b) & 1) - (int)((w >> (32 + b)) & 1);
    return v;
}

static void check_cbd() {
    const uint64_t ones = ~(uint64_t)0, lo = 0xffffffffull, hi = lo << 32;
    for (uint32_t eta = 1; eta <= 32; ++eta) {
        const uint32_t m = agx::sample_eta_mask(eta);
        CHECK(m == (uint32_t)((((uint64_t)1 << eta) - 1)), "eta %u", eta);
        CHECK(agx::sample_cbd(0, m) == 0 && agx::sample_cbd(ones, m) == 0 && agx::sample_cbd(lo, m) == (int)eta && agx::sample_cbd(hi, m) == -(int)eta, "eta %u", eta);
        CHECK(agx::sample_cbd(0xaaaaaaaa55555555ull, m) == cbd_loop(0xaaaaaaaa55555555ull, eta));
        for (int it = 0; it < 300; ++it) {
            const uint64_t w = next64();
            CHECK(agx::sample_cbd(w, m) == cbd_loop(w, eta), "eta %u word %llx", eta, (ull)w);
        }
    }
}

static void check_residue(uint64_t q) {
    for (int v = -32; v <= 32; ++v) {
        const uint64_t got = agx::sample_residue(v, q), want = (uint64_t)((((int64_t)v % (int64_t)q) + (int64_t)q) % (int64_t)q);
        CHECK(got == want, "q=%llu v=%d gave %llu", (ull)q, v, (ull)got);
        if ((uint64_t)(v < 0 ? -v : v) < q) CHECK(got == (v >= 0 ? (uint64_t)v : q - (uint64_t)(-v)));
    }
}

int main(int argc, char** argv) {
    std::vector<uint64_t> moduli;
    for (int i = 1; i < argc; ++i) moduli.push_back(std::strtoull(argv[i], nullptr, 10));
    std::printf("moduli: %zu\n", moduli.size());
    if (moduli.size() < 20) {
        std::printf("FAILED: pass at least 20 moduli\n");
        return 2;
    }
    check_vectors();
    selftest_section("vectors");
    uint8_t bytes[32];
    for (int i = 0; i < 32; ++i) bytes[i] = (uint8_t)next64();
    const agx::sample_key key = key_of(bytes);
    for (uint64_t q : moduli) check_uniform(q, key);
    selftest_section("uniform");
    for (uint64_t q : moduli) check_cap(q);
    selftest_section("cap");
    check_ternary();
    selftest_section("ternary");
    check_cbd();
    selftest_section("cbd");
    for (uint64_t q : moduli) check_residue(q);
    return selftest_report("residue");
}
