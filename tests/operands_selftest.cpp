// operands_selftest.cpp -- csrc/operands.hpp against brute force and at the integer limits, on a CPU (tests/test_operands.py builds and
// runs it; it needs neither HIP nor a GPU).  Prints what it checked; exit status 1 and one line per failure if anything is wrong.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../agilex-ntt_amd/csrc/operands.hpp"
#include "selftest.hpp"

using namespace agx;

// Brute force over frame starts (tests/test_gpu_bench_shapes.py::_touch_expected): a layout overlaps itself iff two distinct frames start
// less than n words apart; the set shifted by off != 0 touches the set iff some frame of one starts less than n words from a frame of
// the other.  Every offset from -extent-2 to extent+2 is asked of partial_overlap, for layouts that do not overlap themselves.
static uint64_t brute_force_grid() {
    const uintptr_t base = (uintptr_t)1 << 40;
    uint64_t cases = 0;
    for (uint32_t n : {2u, 8u})
        for (uint32_t P = 1; P <= 3; ++P)
            for (uint64_t B = 1; B <= 4; ++B)
                for (int64_t ps = 0; ps <= (int64_t)(5 * n * B + 3); ++ps)
                    for (int64_t qs = 0; qs <= (int64_t)(5 * n * P + 3); ++qs) {
                        std::vector<int64_t> starts;
                        for (uint32_t p = 0; p < P; ++p)
                            for (uint64_t b = 0; b < B; ++b) starts.push_back(p * ps + (int64_t)b * qs);
                        bool self = false;
                        for (size_t i = 0; i < starts.size(); ++i)
                            for (size_t j = i + 1; j < starts.size(); ++j) self |= starts[i] - starts[j] < (int64_t)n && starts[j] - starts[i] < (int64_t)n;
                        const int64_t extent = (P - 1) * ps + (int64_t)(B - 1) * qs + n;
                        CHECK(layout_fits(n, P, B, ps, qs));
                        CHECK(self_overlap(n, P, B, ps, qs) == self);
                        ++cases;
                        if (self) continue;
                        cases += 2 * (extent + 2) + 1;      // one per offset
                        // touched[off + extent + 2]: some frame of the set shifted by off starts within n words of a frame of the set
                        std::vector<char> touched(2 * (extent + 2) + 1, 0);
                        for (int64_t s : starts)
                            for (int64_t t : starts)
                                for (int64_t off = s - t - (int64_t)n + 1; off <= s - t + (int64_t)n - 1; ++off) touched[off + extent + 2] = 1;
                        for (int64_t off = -extent - 2; off <= extent + 2; ++off) {
                            const bool want = off != 0 && touched[off + extent + 2];
                            CHECK(partial_overlap(base, base + 8 * (uintptr_t)off, n, P, B, ps, qs) == want);
                        }
                    }
    return cases;
}

static void layout_fits_limits() {
    const int64_t top = (int64_t)1 << 60, max = INT64_MAX;
    // an extent of exactly 2^60 words is accepted, one word more is refused: through either stride, and through n
    CHECK(layout_fits(2, 1, 2, 0, top - 2) && !layout_fits(2, 1, 2, 0, top - 1));
    CHECK(layout_fits(2, 2, 1, top - 2, 0) && !layout_fits(2, 2, 1, top - 1, 0));
    CHECK(layout_fits(32768, 2, 2, top / 2, top / 2 - 32768) && !layout_fits(32768, 2, 2, top / 2, top / 2 - 32767));
    CHECK(layout_fits(2, 3, 0x7fffffffull, (top >> 1) - ((int64_t)1 << 31) + 1, 2) && !layout_fits(2, 3, 0x7fffffffull, (top >> 1) - ((int64_t)1 << 31) + 2, 2));
    // a stride at INT64_MAX counts as soon as a second prime / polynomial uses it; a negative stride is refused whatever the shape
    CHECK(!layout_fits(2, 2, 1, max, 0) && !layout_fits(2, 1, 2, 0, max) && !layout_fits(2, 2, 2, max, max) && !layout_fits(2, 65535, ~0ull, max, max));
    CHECK(layout_fits(2, 1, 1, max, max));      // one frame: no stride is ever applied
    CHECK(!layout_fits(2, 1, 1, -1, 0) && !layout_fits(2, 1, 1, 0, -1) && !layout_fits(2, 2, 2, INT64_MIN, 4) && !layout_fits(2, 1, 0, -1, 0));
    CHECK(layout_fits(2, 2, 0, 0, 0));      // an empty set has no extent
}

// the largest shapes the ABI admits (65,535 primes, the grid limit of 2^31 - 1 polynomials), n = 2
static void largest_shapes() {
    const uintptr_t base = (uintptr_t)1 << 40;
    const uint32_t n = 2, P = 65535;
    const uint64_t B = 0x7fffffffull;
    const int64_t top = (int64_t)1 << 60;
    {   // dense [prime][batch][n]
        const int64_t ps = (int64_t)B * n, qs = n, extent = (int64_t)P * ps;
        CHECK(layout_fits(n, P, B, ps, qs) && !self_overlap(n, P, B, ps, qs));
        CHECK(self_overlap(n, P, B, ps - 1, qs));      // prime 1 starts inside the last polynomial of prime 0
        CHECK(!partial_overlap(base, base, n, P, B, ps, qs));
        for (int64_t off : {(int64_t)1, (int64_t)n, ps, extent - 1})
            CHECK(partial_overlap(base, base + 8 * (uintptr_t)off, n, P, B, ps, qs) && partial_overlap(base + 8 * (uintptr_t)off, base, n, P, B, ps, qs));
        CHECK(!partial_overlap(base, base + 8 * (uintptr_t)extent, n, P, B, ps, qs) && !partial_overlap(base + 8 * (uintptr_t)extent, base, n, P, B, ps, qs));
    }
    {   // the same shape with prime_stride stretched: 65534 does not divide 2^60 - 2 - (B-1) n, so the extent ends within 65534 words of 2^60
        const int64_t qs = n, ps = (top - n - (int64_t)(B - 1) * qs) / (P - 1), extent = (P - 1) * ps + (int64_t)(B - 1) * qs + n;
        CHECK(extent <= top && top - extent < P - 1);
        CHECK(layout_fits(n, P, B, ps, qs) && !layout_fits(n, P, B, ps + 1, qs) && !self_overlap(n, P, B, ps, qs));
        for (int64_t off : {(int64_t)1, (int64_t)(B - 1) * qs + 1, ps - (int64_t)B * qs + 1, ps, (P - 1) * ps, extent - 1})      // into prime 0, its last word, one word into prime 1, ...
            CHECK(partial_overlap(base, base + 8 * (uintptr_t)off, n, P, B, ps, qs) && partial_overlap(base + 8 * (uintptr_t)off, base, n, P, B, ps, qs));
        for (int64_t off : {(int64_t)B * qs, ps - (int64_t)B * qs, extent, extent + 1})      // both ends of the gap behind every prime's polynomials, and past the end
            CHECK(!partial_overlap(base, base + 8 * (uintptr_t)off, n, P, B, ps, qs) && !partial_overlap(base + 8 * (uintptr_t)off, base, n, P, B, ps, qs));
    }
    {   // an extent of exactly 2^60 with every polynomial (3 primes) and with every prime (3 polynomials, off the O(1) paths)
        const int64_t ps3 = (top >> 1) - ((int64_t)1 << 31) + 1;
        CHECK(2 * ps3 + (int64_t)(B - 1) * 2 + 2 == top && layout_fits(n, 3, B, ps3, 2) && !self_overlap(n, 3, B, ps3, 2));
        CHECK(partial_overlap(base, base + 8 * (uintptr_t)(top - 1), n, 3, B, ps3, 2) && !partial_overlap(base, base + 8 * (uintptr_t)top, n, 3, B, ps3, 2));
        const int64_t ps = (int64_t)1 << 44, qs = ps - 1;
        CHECK((P - 1) * ps + 2 * qs + n == top && layout_fits(n, P, 3, ps, qs));
        CHECK(self_overlap(n, P, 3, ps, qs));           // frame (1, 0) starts one word behind frame (0, 1)
        CHECK(!self_overlap(n, P, 3, ps, qs - 1));      // two words behind: they are adjacent
        CHECK(partial_overlap(base, base + 8 * 5, n, P, 3, ps, qs - 1) && !partial_overlap(base, base + 8 * 6, n, P, 3, ps, qs - 1));      // frames sit 0, 2 or 4 words below multiples of 2^44
    }
}

static void ranges() {
    const uintptr_t a = 0x1000;
    CHECK(!ranges_touch(a, 4, a + 32, 4) && !ranges_touch(a + 32, 4, a, 4));      // adjacent
    CHECK(ranges_touch(a, 4, a + 24, 4) && ranges_touch(a + 24, 4, a, 4));        // one shared word
    CHECK(ranges_touch(a, 4, a, 4) && ranges_touch(a, 8, a + 16, 1) && ranges_touch(a + 16, 1, a, 8));      // equal, and one inside the other
    CHECK(!ranges_touch(a, 0, a, 4) && !ranges_touch(a, 4, a, 0) && !ranges_touch(a, 0, a, 0) && !ranges_touch(a + 8, 0, a, 4) && !ranges_touch(a, 4, a + 8, 0));      // empty
    const uintptr_t last = ~(uintptr_t)0 - 7;      // the last aligned word of the address space: a range ending there does not wrap
    CHECK(ranges_touch(last - 24, 4, last, 1) && ranges_touch(last, 1, last - 24, 4));
    CHECK(!ranges_touch(last - 24, 4, 0, 4) && !ranges_touch(0, 4, last - 24, 4) && !ranges_touch(last - 24, 3, last, 1) && !ranges_touch(last, 1, last - 24, 3));
    CHECK(ranges_touch(0, (uint64_t)1 << 61, last, 1));      // the whole address space holds its last word
}

// The buffer rules of agx_ntt_basis_mod_down and agx_ntt_rescale as those calls spelled them out before down_buffers_ok stated the rule once: the
// references below.  true = the call goes on, false = AGX_ERR_BAD_ARGUMENT.
static bool mod_down_rule_as_written(uintptr_t xq, uintptr_t xp, uintptr_t out, uintptr_t scratch, uint64_t qwords, uint64_t pwords) {
    if (out != xq && ranges_touch(out, qwords, xq, qwords)) return false;
    if (ranges_touch(out, qwords, xp, pwords) || ranges_touch(out, qwords, scratch, pwords) || ranges_touch(scratch, pwords, xq, qwords)) return false;
    if (scratch != xp && ranges_touch(scratch, pwords, xp, pwords)) return false;
    return true;
}
static bool rescale_rule_as_written(uintptr_t x, uintptr_t out, uintptr_t scratch, uint64_t slab, uint64_t head) {
    const uintptr_t x_last = x + 8 * head;
    if (out != x && ranges_touch(out, head, x, head + slab)) return false;
    if (ranges_touch(scratch, slab, out, head) || ranges_touch(scratch, slab, x, head)) return false;
    if (scratch != x_last && ranges_touch(scratch, slab, x_last, slab)) return false;
    return true;
}

// down_buffers_ok against both, every placement: slabs of 0 .. 3 words, 1 .. 3 source and target slabs, every base on a grid of 14 words (ranges are
// at most 9 words: equal bases, adjacency and every partial overlap occur).  Rescale is the rule at xq = x, xp = x + 8 qwords, one source slab.
static uint64_t down_buffers_grid() {
    const uintptr_t base = (uintptr_t)1 << 40;
    const int grid = 14;
    uint64_t cases = 0;
    auto at = [&](int w) { return base + 8 * (uintptr_t)w; };
    for (uint64_t slab = 0; slab <= 3; ++slab)
        for (uint32_t T = 1; T <= 3; ++T) {
            for (uint32_t S = 1; S <= 3; ++S)
                for (int xq = 0; xq < grid; ++xq)
                    for (int xp = 0; xp < grid; ++xp)
                        for (int out = 0; out < grid; ++out)
                            for (int scratch = 0; scratch < grid; ++scratch, ++cases)
                                CHECK(down_buffers_ok(at(xq), T * slab, at(xp), S * slab, at(out), at(scratch)) ==
                                      mod_down_rule_as_written(at(xq), at(xp), at(out), at(scratch), T * slab, S * slab));
            const uint64_t head = T * slab;      // a plan of P = T + 1 primes
            for (int x = 0; x < grid; ++x)
                for (int out = 0; out < grid; ++out)
                    for (int scratch = 0; scratch < grid; ++scratch, ++cases)
                        CHECK(down_buffers_ok(at(x), head, at(x) + 8 * head, slab, at(out), at(scratch)) == rescale_rule_as_written(at(x), at(out), at(scratch), slab, head));
        }
    return cases;
}

// The scratch rule of agx_ntt_basis_quotient, agx_ntt_plain_scale_down / _reduce, agx_ntt_ckks_decode and agx_ntt_batch_decode as those calls spelled it out
// before scratch_buffers_ok stated it once.  true = the call goes on, false = AGX_ERR_BAD_ARGUMENT.
static bool scratch_rule_as_written(uintptr_t x, uintptr_t scratch, uintptr_t out, uint64_t x_words, uint64_t out_words) {
    if (scratch != x && ranges_touch(scratch, x_words, x, x_words)) return false;
    if (ranges_touch(out, out_words, x, x_words) || ranges_touch(out, out_words, scratch, x_words)) return false;
    return true;
}

// scratch_buffers_ok against it, every placement: x and the scratch of 0 .. 6 words, out of 0 .. 3, every base on a grid of 14 words (equal bases,
// adjacency and every partial overlap occur); then by hand: the scratch that IS x, empty ranges, ranges ending at the top of the address space.
static uint64_t scratch_buffers_grid() {
    const uintptr_t base = (uintptr_t)1 << 40;
    const int grid = 14;
    uint64_t cases = 0;
    auto at = [&](int w) { return base + 8 * (uintptr_t)w; };
    for (uint64_t x_words : {0, 1, 2, 3, 4, 6})
        for (uint64_t out_words = 0; out_words <= 3; ++out_words)
            for (int x = 0; x < grid; ++x)
                for (int scratch = 0; scratch < grid; ++scratch)
                    for (int out = 0; out < grid; ++out, ++cases)
                        CHECK(scratch_buffers_ok(at(x), x_words, at(scratch), at(out), out_words) == scratch_rule_as_written(at(x), at(scratch), at(out), x_words, out_words));
    const uintptr_t a = 0x1000;
    CHECK(scratch_buffers_ok(a, 4, a, a + 32, 2) && scratch_buffers_ok(a, 4, a, a - 16, 2));      // in place, out adjacent on either side
    CHECK(!scratch_buffers_ok(a, 4, a, a + 24, 2) && !scratch_buffers_ok(a, 4, a, a, 2) && !scratch_buffers_ok(a, 4, a, a - 8, 2));      // out on the shared words
    CHECK(!scratch_buffers_ok(a, 4, a + 8, a + 64, 2) && !scratch_buffers_ok(a, 4, a - 24, a + 64, 2));      // a scratch that straddles x
    CHECK(scratch_buffers_ok(a, 4, a + 32, a + 64, 2) && !scratch_buffers_ok(a, 4, a + 32, a + 56, 2) && !scratch_buffers_ok(a, 4, a + 32, a + 16, 2));      // apart; out on the scratch, on x
    CHECK(scratch_buffers_ok(a, 0, a + 8, a, 2) && scratch_buffers_ok(a, 4, a + 32, a + 8, 0) && scratch_buffers_ok(a, 0, a, a, 0));      // empty ranges touch nothing
    const uintptr_t last = ~(uintptr_t)0 - 7;      // the last aligned word of the address space: a range ending there does not wrap
    CHECK(scratch_buffers_ok(last - 24, 4, last - 56, 0, 2) && scratch_buffers_ok(0, 2, 16, last - 24, 4));
    CHECK(!scratch_buffers_ok(last - 24, 4, last - 56, last, 1) && !scratch_buffers_ok(last - 24, 4, last - 48, 0, 2) && scratch_buffers_ok(last - 24, 4, last - 24, 0, 2));
    return cases;
}

int main() {
    const uint64_t cases = brute_force_grid();
    std::printf("brute force: %" PRIu64 " cases\n", cases);
    std::printf("down_buffers_ok: %" PRIu64 " placements\n", down_buffers_grid());
    std::printf("scratch_buffers_ok: %" PRIu64 " placements\n", scratch_buffers_grid());
    layout_fits_limits();
    largest_shapes();
    ranges();
    return selftest_report("operand predicates");
}
