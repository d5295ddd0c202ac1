// selftest.hpp -- what the stand-alone CPU programs tests/*_selftest.cpp share: the CHECK macro with its counters, the splitmix64 generator, mulmod
// in unsigned __int128, and the report lines tests/test_selftests.py reads.  Each program keeps its own main and is built from its own sources alone.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>

typedef unsigned __int128 u128;

static long g_checks = 0, g_failures = 0, g_reported = 0;

// the optional printf-style detail of a failed CHECK
inline void selftest_detail() {}
__attribute__((format(printf, 1, 2))) inline void selftest_detail(const char* fmt, ...) {
    std::printf(": ");
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
}

// CHECK(cond) or CHECK(cond, "format", ...): counts the check; the first 20 failures print one line each with the condition and the detail
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        ++g_checks;                                                             \
        if (!(cond) && ++g_failures <= 20) {                                    \
            std::printf("FAIL %s:%d: %s", __FILE__, __LINE__, #cond);           \
            selftest_detail(__VA_ARGS__);                                       \
            std::printf("\n");                                                  \
        }                                                                       \
    } while (0)

static uint64_t g_rng = 0x243F6A8885A308D3ull;      // a program that wants another sequence assigns its seed first thing in main
inline uint64_t next64() {      // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline u128 next128() { return ((u128)next64() << 64) | next64(); }

inline uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((u128)a * b % q); }

// "<name>: N checks" for the checks made since the last such line
inline void selftest_section(const char* name) {
    std::printf("%s: %ld checks\n", name, g_checks - g_reported);
    g_reported = g_checks;
}

// the last section's line, then "ok: 0 failures" or "FAILED: N failures"; returns main's exit status
inline int selftest_report(const char* name) {
    selftest_section(name);
    std::printf("%s: %ld failures\n", g_failures ? "FAILED" : "ok", g_failures);
    return g_failures ? 1 : 0;
}
