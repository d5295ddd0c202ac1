// q60c_class_selftest.cpp -- stand-alone CPU program (own main; tests/test_selftests.py builds and runs it under the sanitizers): the two questions
// csrc/q60c_class.hpp answers about a plan's moduli, against their definitions.  q60c_of: c for q = 2^60 - c with 0 < c < 2^28, 0 otherwise, on both edges.
// q60c_skip_class, the per-plan flag that makes registry id 165 launch its skip-form kernel: true exactly when EVERY modulus has 0 < c <= 2^27 -- one
// modulus outside, as first, last or any middle entry of the set, clears it, so a flag taken from one end of the list alone would show here.
#include <vector>

#include "../agilex-ntt_amd/csrc/q60c_class.hpp"
#include "selftest.hpp"

using namespace agx;

int main() {
    const uint64_t top = 1ull << 60;
    static_assert(kQ60cSkipMaxC == (1u << 27), "the class limit");
    // q60c_of on the edges of its class
    CHECK(q60c_of(top) == 0 && q60c_of(top + 1) == 0 && q60c_of(top - 1) == 1);
    CHECK(q60c_of(top - ((1ull << 28) - 1)) == (1u << 28) - 1 && q60c_of(top - (1ull << 28)) == 0 && q60c_of(0) == 0 && q60c_of(~0ull) == 0);
    for (int k = 0; k < 100000; ++k) {
        const uint64_t c = next64() >> (36 + next64() % 28);      // widths 1 .. 28 bits
        const uint64_t q = top - c;
        CHECK(q60c_of(q) == (c > 0 && c < (1ull << 28) ? (uint32_t)c : 0u), "c = %llu", (unsigned long long)c);
    }
    // the flag: brute force over sets of 1 .. 6 moduli with any subset of positions outside the skip class
    const uint64_t inside[] = {top - 1, top - 16383, top - 245759, top - (1ull << 26), top - ((1ull << 27) - 1), top - (1ull << 27)};
    const uint64_t outside[] = {top - ((1ull << 27) + 1), top - ((1ull << 27) + 8191), top - ((1ull << 28) - 1), top - (1ull << 28), top, (1ull << 59) + 1, 65537};
    CHECK(!q60c_skip_class(nullptr, 0));
    for (uint32_t count = 1; count <= 6; ++count)
        for (uint32_t mask = 0; mask < (1u << count); ++mask)
            for (int rep = 0; rep < 40; ++rep) {
                std::vector<uint64_t> m(count);
                for (uint32_t i = 0; i < count; ++i) m[i] = (mask >> i & 1) ? outside[next64() % 7] : inside[next64() % 6];
                CHECK(q60c_skip_class(m.data(), count) == (mask == 0), "count %u mask %u", count, mask);
            }
    return selftest_report("q60c_class");
}
