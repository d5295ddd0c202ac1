// moddown_rb2_body.hpp -- the body of moddown_rb2 (AGX_RESCALE_FLOOR) and moddown_round_rb2 (AGX_RESCALE_ROUND), rb_kernels.hpp: ONE text, included inside
// both kernels' braces.  Not a header in the usual sense: no include guard, nothing at namespace scope.  The including kernel has the template parameters
// L, R, PPB, ARITH, the arguments xq, y, out, consts, mat, dall, tw_rb, pairs_per_prime, frames_x, prime_stride, poly_stride, num_src, dst_first, num_dst,
// and in scope
//   constexpr bool ROUND;  const ulonglong2* rsrc ([S] {c_i = h D_i^-1 mod q_i, q_i});  const uint64_t* rdst ([T] t h mod q_j)
// -- the last two are arguments of moddown_round_rb2 and constant null pointers in moddown_rb2, where no statement that names them is instantiated.
// Why an included text and not an inlined function: with the body in a __forceinline__ function template, the FLOOR kernels no longer compiled to the
// assembly they had (about 770 of the 8,665 lines of an n = 2048 instance were scheduled differently); included, they do, which
// tools/compare_device_asm.py proves (profiles/r14_mod_down_modes_device_asm.txt).  FLOOR must launch exactly the code it launched before ROUND existed.
using F = frame_of<L, R, ARITH>;
constexpr int C = F::C, T = F::T;
static_assert(T >= 64, "one frame must span whole waves");
F f;
f.tid = threadIdx.x & (T - 1);
const uint32_t slot = PPB == 1 ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / T));      // a frame spans whole waves: wave-uniform
uint32_t group = blockIdx.x / num_dst;      // out of the vector unit: pinned to a scalar register (extend_rb2)
asm volatile("" : "+s"(group));
const uint32_t j = blockIdx.x - group * num_dst;
uint64_t fx = (uint64_t)group * PPB + slot;
const bool live = fx < frames_x;
if (!live) fx = frames_x - 1;                         // keep every thread on the barriers
const uint32_t prime = dst_first + j;
const uint64_t q = consts[prime].q, q2 = q << 1;
f.init_consts(q, consts[prime].est);
// q <= 2^60: rescale_finish takes both operands in [0,4q), so the transform may skip its last conditional subtracts and xq_j needs no reduction
f.lazy_out = F::LAZY16;
f.slab = reinterpret_cast<uint64_t*>(agx_dyn_lds) + (size_t)slot * F::slab_elems;
int64_t base = (int64_t)j * prime_stride + (int64_t)fx * poly_stride;
constexpr int GRP = 4, NG = C / GRP;      // registers per group of loads (y: GRP words; xq: two 16-byte loads), groups per thread
static_assert(C % GRP == 0 && NG % 2 == 0, "whole groups, and group 0 of every source in buffer 0");
const uint64_t* yf = y + (int64_t)fx * poly_stride;      // the frame under source 0 (wave-uniform: lanes add tid)
asm volatile("" : "+s"(base), "+s"(yf));      // wave-uniform, scalar registers of their own (extend_rb2)
const ulonglong2* row = mat + (size_t)j * num_src;
uint64_t acc[C];
{
    uint64_t z[2][GRP];
#pragma unroll
    for (int r = 0; r < C; ++r) acc[r] = 0;
    static_for<0, GRP>([&](auto I) { z[0][I] = yf[f.tid + (uint32_t)(int)I * T]; });
    for (uint32_t i = 0; i < num_src; ++i) {      // wave-uniform
        const ulonglong2 c = row[i];
        [[maybe_unused]] const ulonglong2 rs = ROUND ? rsrc[i] : ulonglong2{};      // {c_i, q_i}: wave-uniform; FLOOR reads nothing
        const uint64_t* cur = yf + (int64_t)i * prime_stride;
        const uint64_t* nxt = yf + (int64_t)(i + 1 < num_src ? i + 1 : i) * prime_stride;      // behind the last source: its own first group again (a cache hit, dropped)
        static_for<0, NG>([&](auto Gq) {
            constexpr int g = Gq;
            const uint64_t* pg = g + 1 < NG ? cur + (uint32_t)((g + 1) * GRP) * T : nxt;      // opaque and scalar: every group shares the GRP lane offsets (extend_rb2)
            asm volatile("" : "+s"(pg));
            static_for<0, GRP>([&](auto I) { z[(g + 1) & 1][I] = pg[f.tid + (uint32_t)(int)I * T]; });
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, GRP>([&](auto I) {
                constexpr int r = g * GRP + (int)I;
                asm volatile("" : "+v"(acc[r]));
                if constexpr (ROUND) acc[r] = basis_accumulate(acc[r], moddown_round_y(z[g & 1][I], rs.x, rs.y), c.x, c.y, q, q2);
                else acc[r] = basis_accumulate(acc[r], z[g & 1][I], c.x, c.y, q, q2);
                asm volatile("" : "+v"(acc[r]));
            });
            __builtin_amdgcn_sched_barrier(0);
        });
    }
}
if constexpr (ROUND) {
    const uint64_t hq = rdst[j];      // t h mod q_j: wave-uniform
#pragma unroll
    for (int r = 0; r < C; ++r) acc[r] = moddown_round_acc(acc[r], hq, q);
}
const ulonglong2 d = dall[j];      // {D^-1 mod q_j, quotient}: wave-uniform
constexpr bool EARLY = !F::STREAM_TW && !F::SPLIT && F::NP >= 2 && NG <= 2;      // as mulhat_rb2 / rescale_rb2
const bhat_pair* xp = reinterpret_cast<const bhat_pair*>(xq + base + (uint32_t)f.tid * C);
bhat_pair w[EARLY ? NG : 2][GRP / 2];
auto request = [&](auto Gq) {
    constexpr int g = Gq;
    static_for<0, GRP / 2>([&](auto I) { w[EARLY ? g : (g & 1)][I] = xp[g * (GRP / 2) + (int)I]; });
};
if constexpr (EARLY) {
    f.template forward_passes<0, F::NP - 1>(acc, tw_rb + (size_t)prime * pairs_per_prime);
    static_for<0, NG>(request);
    f.template forward_passes<F::NP - 1, F::NP>(acc, tw_rb + (size_t)prime * pairs_per_prime);
} else {
    f.forward(acc, tw_rb + (size_t)prime * pairs_per_prime);
    request(std::integral_constant<int, 0>{});
}
static_for<0, NG>([&](auto Gq) {
    constexpr int g = Gq;
    if constexpr (!EARLY && g + 1 < NG) request(std::integral_constant<int, g + 1>{});
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, GRP>([&](auto I) {
        constexpr int i = I, r = g * GRP + i;
        uint64_t v = w[EARLY ? g : (g & 1)][i / 2][i & 1];
        // beyond 2^60 the difference wants xq_j (lazy: below 4q, which may not fit 64 bits -- reduce_4q never forms it) and the transform's
        // result, which is then fully reduced, below q
        if constexpr (!F::LAZY16) v = reduce_4q(v, q, q2);
        asm volatile("" : "+v"(acc[r]));
        acc[r] = rescale_finish<F::LAZY16>(v, acc[r], d.x, d.y, q);
        asm volatile("" : "+v"(acc[r]));
    });
    __builtin_amdgcn_sched_barrier(0);
});
f.store_last_layout(acc, out, base, live);
