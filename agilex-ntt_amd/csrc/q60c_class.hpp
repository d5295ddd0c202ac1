// q60c_class.hpp -- the classes of moduli 2^60 - c as device arithmetic (modarith.hpp) and host code (agx_ntt.cpp) both read them: the limit of the skip
// form, and the two questions the host asks of a plan's moduli.  Plain C++, no HIP: tests/q60c_class_selftest.cpp compiles it alone.
#pragma once
#include <cstdint>

namespace agx {

// Moduli 2^60 - c with 0 < c <= this limit may take the skip form of the two-twiddle butterfly (reduction on every second stage, lazy-range constant 7q).
// modarith.hpp (q60c_skip_bounds) proves the form's bounds for exactly this class, prepare_plan_image (agx_ntt.cpp) tests a plan's moduli against it.
// (The bounds hold up to c = 2^27 + 1; the power of two is the class.)
constexpr uint32_t kQ60cSkipMaxC = 1u << 27;

// c of a modulus q = 2^60 - c with 0 < c < 2^28 (arithmetic level 3), or 0 for any other modulus
inline uint32_t q60c_of(uint64_t q) {
    const uint64_t top = 1ull << 60;
    return q < top && top - q < (1ull << 28) ? (uint32_t)(top - q) : 0u;
}

// The per-plan flag of the skip form (plan_view::q60c_skip): EVERY modulus is 2^60 - c with 0 < c <= kQ60cSkipMaxC.  One modulus outside, wherever it
// stands, and the plan keeps the every-stage kernel.
inline bool q60c_skip_class(const uint64_t* moduli, uint32_t count) {
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t c = q60c_of(moduli[k]);
        if (c == 0 || c > kQ60cSkipMaxC) return false;
    }
    return count > 0;
}

}  // namespace agx
