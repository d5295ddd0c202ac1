// agx_ntt.cpp -- the extern "C" boundary declared in include/agx_ntt.h.
// Owns argument validation, plan objects (device tables, the routes from a call to its kernel) and the mapping of HIP errors to
// status codes.  Kernels live in ntt_kernels.hip and the registry groups; number theory in host_math.cpp; host-resident frames in agx_host.cpp.
#include "../../include/agx_ntt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "host_math.hpp"
#include "operands.hpp"
#include "plan_internal.hpp"
#include "rb_registry.hpp"
#ifdef AGX_DIAG
#include "../../tools/agx_ntt_diag.h"
#endif

using namespace agx;

thread_local int g_last_hip_error = 0;

namespace agx {
int& last_hip_error_slot() { return g_last_hip_error; }
int hip_fail(hipError_t e) {
    g_last_hip_error = (int)e;
    return e == hipErrorOutOfMemory ? AGX_ERR_ALLOC : AGX_ERR_HIP;
}
}  // namespace agx

namespace {

// function attributes (large dynamic LDS) are per device and never change: set them once per device,
// not on every plan creation
hipError_t kernels_init_once(int device) {
    static std::once_flag once[kMaxDevices];
    static hipError_t result[kMaxDevices];
    if (device < 0 || device >= kMaxDevices) return kernels_init();
    std::call_once(once[device], [device] { result[device] = kernels_init(); });
    return result[device];
}

uint32_t* plan_ticket_for(void* ctx, hipStream_t s) {
    const agx_ntt_plan* p = static_cast<const agx_ntt_plan*>(ctx);
    if (!p->d_ticket) return nullptr;
    // hipStreamPerThread is ONE handle value that names a different stream in every host thread: two threads launching on "it" run
    // concurrently and must not share a pair.  No pair is provably free for it: stateless fixed-stride kernels.
    if (s == hipStreamPerThread) return nullptr;
    std::lock_guard<std::mutex> lock(p->ticket_mu);
    for (size_t i = 0; i < p->ticket_streams.size(); ++i)
        if (p->ticket_streams[i] == s) {
            p->ticket_pending[i] = 1;
            return p->d_ticket + 2 * i;
        }
    size_t slot = p->ticket_streams.size();
    if (slot >= kTicketSlots) {
        // every slot is taken: one whose stream's latest ticket launch has completed is idle -- its pair is zero again -- and can change hands
        slot = kTicketSlots;
        for (size_t i = 0; i < kTicketSlots && slot == kTicketSlots; ++i)
            if (!p->ticket_pending[i] && p->ticket_events[i] && hipEventQuery(p->ticket_events[i]) == hipSuccess) slot = i;
        if (slot == kTicketSlots) return nullptr;      // all busy: the stateless kernels
        p->ticket_streams[slot] = s;
    } else {
        p->ticket_streams.push_back(s);      // capacity reserved at plan creation: no allocation here
    }
    if (!p->ticket_events[slot] && hipEventCreateWithFlags(&p->ticket_events[slot], hipEventDisableTiming) != hipSuccess) {
        p->ticket_events[slot] = nullptr;      // without an event the slot can never be proven idle: it simply stays with this stream
    }
    p->ticket_pending[slot] = 1;
    return p->d_ticket + 2 * slot;
}

void plan_ticket_launched(void* ctx, hipStream_t s, uint32_t* pair) {
    const agx_ntt_plan* p = static_cast<const agx_ntt_plan*>(ctx);
    if (!pair || !p->d_ticket) return;
    const size_t slot = (size_t)(pair - p->d_ticket) / 2;
    std::lock_guard<std::mutex> lock(p->ticket_mu);
    if (slot >= p->ticket_events.size()) return;
    if (p->ticket_events[slot] && hipEventRecord(p->ticket_events[slot], s) != hipSuccess) {
        (void)hipEventDestroy(p->ticket_events[slot]);
        p->ticket_events[slot] = nullptr;
    }
    p->ticket_pending[slot] = 0;
}

// n^-1 mod q for odd q and n a power of two: ((q+1)/2)^log2(n)
uint64_t inv_pow2_mod(uint32_t log_n, uint64_t q) {
    const uint64_t half = (q + 1) >> 1;
    uint64_t r = 1 % q;
    for (uint32_t i = 0; i < log_n; ++i) r = mul_mod(r, half, q);
    return r;
}

}  // namespace

namespace agx {

int check_size(uint32_t n) {
    return (n >= AGX_NTT_MIN_N && n <= AGX_NTT_MAX_N && is_pow2(n)) ? AGX_OK : AGX_ERR_BAD_SIZE;
}

// what the butterfly arithmetic needs (src/kernel/ntt.cpp:302-369): 4q < 2^64 and 2n | q-1
int check_modulus(uint64_t q, uint32_t n) {
    if (q < 3 || (q & 1) == 0 || q >= (1ull << 62)) return AGX_ERR_BAD_MODULUS;
    if ((q - 1) % (2ull * n)) return AGX_ERR_BAD_MODULUS;
    return AGX_OK;
}

int check_shape(uint32_t n, uint32_t num_primes) {
    if (int rc = check_size(n)) return rc;
    return num_primes == 0 || num_primes > 65535 ? AGX_ERR_BAD_ARGUMENT : AGX_OK;
}

int check_create_args(uint32_t n, uint32_t num_primes, const uint64_t* moduli, const uint64_t* tw, const uint64_t* pre, const uint64_t* itw, const uint64_t* ipre) {
    if (!moduli || !tw || !pre || (itw == nullptr) != (ipre == nullptr)) return AGX_ERR_NULL_POINTER;
    if (int rc = check_shape(n, num_primes)) return rc;
    for (uint32_t k = 0; k < num_primes; ++k)
        if (int rc = check_modulus(moduli[k], n)) return rc;
    return AGX_OK;
}

// Plan rule: there is a plan, and its tables (and any staging memory of the call) live on the current device.
int check_plan(const agx_ntt_plan* plan) {
    if (!plan) return AGX_ERR_NULL_POINTER;
    int dev = -1;
    return hipGetDevice(&dev) == hipSuccess && dev == plan->device ? AGX_OK : AGX_ERR_BAD_ARGUMENT;
}

void free_plan(agx_ntt_plan* p) {
    if (!p) return;
    for (hipEvent_t ev : p->ticket_events)
        if (ev) (void)hipEventDestroy(ev);
    delete p;      // the device memory goes with its owners
}

// the pass tables of `e` for every prime, from natural-index {w, w'} tables ([num_primes][n]) of one direction; what a slot holds is the
// entry's business (rb_entry::build), which is why it is told the modulus
static std::vector<ulonglong2> build_pass_table(const rb_entry* e, const std::vector<ulonglong2>& pairs, const std::vector<uint64_t>& moduli, uint32_t n) {
    const uint32_t num_primes = (uint32_t)moduli.size();
    std::vector<ulonglong2> out;
    std::vector<uint64_t> w(n), wp(n);
    for (uint32_t k = 0; k < num_primes; ++k) {
        for (uint32_t j = 0; j < n; ++j) w[j] = pairs[(size_t)k * n + j].x, wp[j] = pairs[(size_t)k * n + j].y;
        e->build(w.data(), wp.data(), moduli[k], out);
    }
    return out;
}

// The ONE place that decides which registry entry serves which call, from the plan's variant, entry and tables; called when a plan is
// instantiated and at the end of agx_ntt_plan_set_variant.  LDS_RADIX2 (or no entry): every route is generic.  forward_large: the tuned
// default's companion; an explicit id applies to every call.  inverse / polymul / polymul_ntt take the entry only if it has that launcher
// and the plan has inverse pass tables; the entry points spell out the fallbacks.
static void resolve_routes(agx_ntt_plan* p) {
    route generic;
    generic.n = p->n, generic.log_n = p->log_n, generic.num_primes = p->num_primes;
    generic.consts = p->d_consts, generic.tw = p->d_tw, generic.itw = p->d_itw, generic.rescale = p->d_rescale;
    generic.ticket_for = &plan_ticket_for, generic.ticket_launched = &plan_ticket_launched;
    generic.ticket_ctx = p;      // the plan is heap-allocated and never moves
    auto through = [&](const pass_tables& t) {
        route r = generic;
        r.rb = t.entry, r.tw_rb = t.fwd, r.itw_rb = t.inv;
        return r;
    };
    const rb_entry* e = p->variant == AGX_VARIANT_LDS_RADIX2 ? nullptr : p->main.entry;
    const route main = e ? through(p->main) : generic;
    const bool inv = e && p->main.inv;
    plan_routes& r = p->routes;
    r.forward = main;
    const bool large = e && !p->explicit_id && p->chosen.forward_large && p->chosen.forward_large == p->companion.entry;
    r.forward_large = large ? through(p->companion) : route{};
    r.min_frames = p->chosen.min_frames;
    r.inverse = inv && e->launch_inv ? main : generic;
    r.polymul = inv && e->launch_mul ? main : generic;
    r.polymul_ntt = inv && e->launch_mulhat ? main : generic;
    // the fused second launch pairs with whatever `inverse` is; everything else (n <= 512, the 32-bit families, radix-2) is generic: the
    // call then runs `inverse`, the coefficient-domain step and `forward` on views of these routes
    r.rescale = inv && e->launch_rescale ? main : generic;
    r.extend = e && e->launch_extend ? main : generic;      // forward tables only
    r.moddown = inv && e->launch_moddown ? main : generic;      // pairs with `inverse` on the source primes, as rescale does on the last
}

static const route& forward_route(const agx_ntt_plan* p, uint64_t batch) {
    const plan_routes& r = p->routes;
    return r.forward_large.rb && batch * p->num_primes >= r.min_frames ? r.forward_large : r.forward;
}

// c of a modulus q = 2^60 - c with 0 < c < 2^28, or 0 for any other modulus
static uint32_t q60c_of(uint64_t q) {
    const uint64_t top = 1ull << 60;
    return q < top && top - q < (1ull << 28) ? (uint32_t)(top - q) : 0u;
}

void prepare_plan_image(plan_image& img, uint32_t n, uint32_t num_primes, const uint64_t* moduli, const uint64_t* psi,
                        const uint64_t* tw, const uint64_t* pre, const uint64_t* itw, const uint64_t* ipre) {
    img.n = n;
    img.log_n = (uint32_t)log2u(n);
    img.num_primes = num_primes;
    img.has_inverse = itw != nullptr;
    img.moduli.assign(moduli, moduli + num_primes);
    img.psi.assign(num_primes, 0);
    if (psi) img.psi.assign(psi, psi + num_primes);
    img.consts.assign(num_primes, prime_consts{});
    img.tw_pairs.resize((size_t)num_primes * n);
    if (itw) img.itw_pairs.resize((size_t)num_primes * n);
    // The fast butterfly is only value-equivalent to the reference's when every modulus is <= 2^61
    // and the tables honour the contract precon[j] = floor(twiddle[j] * 2^64 / q), twiddle[j] < q.
    // Tables that do not (e.g. the placeholders of the reference's main.cpp:49-55) get the exact
    // kernels, which repeat the reference's operations mod 2^64 whatever they are fed.
    // level 3 (on top of level 2): every modulus is 2^60 - c with 0 < c < 2^28 (the forward kernels specialised for this class, modarith.hpp)
    img.arith_level = 3;
    for (uint32_t k = 0; k < num_primes && img.arith_level > 0; ++k) {
        const uint64_t q = moduli[k];
        if (!q60c_of(q)) img.arith_level = std::min(img.arith_level, 2);
        if (q > (1ull << 60)) img.arith_level = std::min(img.arith_level, 1);
        if (q > (1ull << 61)) img.arith_level = 0;
        for (uint32_t j = 1; j < n && img.arith_level > 0; ++j) {
            const uint64_t w = tw[(size_t)k * n + j];
            if (w >= q || pre[(size_t)k * n + j] != shoup_quotient(w, q)) img.arith_level = 0;
            // the inverse kernels of a plan use the same arithmetic form: its tables must honour the contract too
            if (itw && img.arith_level > 0) {
                const uint64_t iw = itw[(size_t)k * n + j];
                if (iw >= q || ipre[(size_t)k * n + j] != shoup_quotient(iw, q)) img.arith_level = 0;
            }
        }
    }
    img.narrow_level = 2;
    for (uint32_t k = 0; k < num_primes; ++k) {
        if (moduli[k] >= (1ull << 30)) img.narrow_level = std::min(img.narrow_level, 1);
        if (moduli[k] >= (1ull << 31)) img.narrow_level = 0;
    }
    img.chosen = regblock_select(n, -1, img.arith_level, img.narrow_level);
    for (uint32_t k = 0; k < num_primes; ++k) {
        const uint64_t q = moduli[k];
        prime_consts& c = img.consts[k];
        std::memset(&c, 0, sizeof(c));
        c.q = q;
        const unsigned __int128 mu = ~(unsigned __int128)0 / q;  // = floor(2^128 / q) for odd q > 1
        c.mu_hi = (uint64_t)(mu >> 64);
        c.mu_lo = (uint64_t)mu;
        if (q >= (1ull << 58) && q <= (1ull << 60)) {
            // reduce_final_est (modarith.hpp) needs v < 16q <= 2^64: only the 16q-lazy kernels (arith level 2, q <= 2^60) call it, and
            // the estimate is only ever set for moduli they accept, so a wider modulus can never reach that path with est != 0
            // float slightly below 2^32 / q (reduce_final_est): scaled down by 2^-20, then rounded toward zero
            float f = (float)(4294967296.0 / (double)q * (1.0 - 1.0 / 1048576.0));
            if ((double)f > 4294967296.0 / (double)q * (1.0 - 1.0 / 1048576.0)) f = std::nextafterf(f, 0.0f);
            uint32_t bits;
            std::memcpy(&bits, &f, sizeof(bits));
            c.est = bits;
        }
        c.est |= (uint64_t)q60c_of(q) << 32;

        c.n_inv = inv_pow2_mod(img.log_n, q);
        c.n_inv_p = shoup_quotient(c.n_inv, q);
        const uint64_t* twk = tw + (size_t)k * n;
        const uint64_t* prek = pre + (size_t)k * n;
        for (uint32_t j = 0; j < n; ++j) img.tw_pairs[(size_t)k * n + j] = make_ulonglong2(twk[j], prek[j]);
        if (itw) {
            const uint64_t* itwk = itw + (size_t)k * n;
            const uint64_t* iprek = ipre + (size_t)k * n;
            for (uint32_t j = 0; j < n; ++j) img.itw_pairs[(size_t)k * n + j] = make_ulonglong2(itwk[j], iprek[j]);
            c.w1n = mul_mod(itwk[1] % q, c.n_inv, q);
            c.w1n_p = shoup_quotient(c.w1n, q);
        }
    }
    // agx_ntt_rescale: q_L^-1 mod q_i with its quotient, h mod q_i and h = (q_L - 1) / 2, for i < P-1
    img.rescale_legal = num_primes >= 2;
    img.rescale.assign(num_primes >= 2 ? num_primes - 1 : 0, rescale_consts{});
    for (uint32_t k = 0; k + 1 < num_primes; ++k) {
        const uint64_t q = moduli[k], q_last = moduli[num_primes - 1], h = (q_last - 1) >> 1;
        rescale_consts& rc = img.rescale[k];
        rc.q_last = q_last, rc.h = h, rc.h_mod_q = h % q;
        if (inv_mod_euclid(q_last, q, &rc.qlinv)) rc.qlinv_p = shoup_quotient(rc.qlinv, q);
        else img.rescale_legal = false;
    }
    const rb_selection& c = img.chosen;
    if (c.main) img.tables.push_back({c.main, build_pass_table(c.main, img.tw_pairs, img.moduli, n), itw ? build_pass_table(c.main, img.itw_pairs, img.moduli, n) : std::vector<ulonglong2>{}});
    if (c.forward_large && c.forward_large != c.main) img.tables.push_back({c.forward_large, build_pass_table(c.forward_large, img.tw_pairs, img.moduli, n), {}});
}

static int upload_pass_tables(pass_tables& dst, const host_pass_tables& src) {
    dst.entry = src.entry;
    if (int rc = dst.fwd.upload(src.fwd)) return rc;
    return src.inv.empty() ? AGX_OK : dst.inv.upload(src.inv);
}

int prepare_auto_image(plan_image& img, uint32_t n, uint32_t num_primes, const uint64_t* moduli, const uint64_t* psi) {
    std::vector<uint64_t> roots(num_primes), tw((size_t)num_primes * n), pre(tw.size()), itw(tw.size()), ipre(tw.size());
    for (uint32_t k = 0; k < num_primes; ++k) {
        const uint64_t q = moduli[k];
        if (int rc = check_modulus(q, n)) return rc;
        if (!is_prime_u64(q)) return AGX_ERR_BAD_MODULUS;
        roots[k] = psi ? psi[k] : min_primitive_root_2n(q, n);
        if (!is_primitive_root_2n(roots[k], q, n)) return AGX_ERR_BAD_ROOT;
        power_tables_bitrev(q, roots[k], n, &tw[(size_t)k * n], &pre[(size_t)k * n]);
        power_tables_bitrev(q, inv_mod(roots[k], q), n, &itw[(size_t)k * n], &ipre[(size_t)k * n]);
    }
    prepare_plan_image(img, n, num_primes, moduli, roots.data(), tw.data(), pre.data(), itw.data(), ipre.data());
    return AGX_OK;
}

int instantiate_plan(agx_ntt_plan** out, const plan_image& img) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return AGX_ERR_NO_DEVICE;
    std::unique_ptr<agx_ntt_plan, void (*)(agx_ntt_plan*)> p(new (std::nothrow) agx_ntt_plan, &free_plan);
    if (!p) return AGX_ERR_ALLOC;
    p->n = img.n, p->log_n = img.log_n, p->num_primes = img.num_primes;
    p->has_inverse = img.has_inverse, p->arith_level = img.arith_level, p->narrow_level = img.narrow_level;
    p->chosen = img.chosen;
    p->rescale_legal = img.rescale_legal;
    p->ticket_streams.reserve(kTicketSlots);      // plan_ticket_for() runs inside unguarded launch calls: it must never allocate
    p->ticket_events.assign(kTicketSlots, nullptr);
    p->ticket_pending.assign(kTicketSlots, 0);
    p->moduli = img.moduli;
    p->psi = img.psi;
    int rc = AGX_OK;
    AGX_HIP(hipGetDevice(&p->device));
    AGX_HIP(kernels_init_once(p->device));
    if ((rc = p->d_consts.upload(img.consts))) return rc;
    if (!img.rescale.empty() && (rc = p->d_rescale.upload(img.rescale))) return rc;
    if ((rc = p->d_ticket.upload(std::vector<uint32_t>(2 * kTicketSlots, 0)))) return rc;
    if ((rc = p->d_tw.upload(img.tw_pairs))) return rc;
    if (img.has_inverse && (rc = p->d_itw.upload(img.itw_pairs))) return rc;
    for (const host_pass_tables& t : img.tables)
        if ((rc = upload_pass_tables(t.entry == img.chosen.main ? p->main : p->companion, t))) return rc;
    resolve_routes(p.get());
    *out = p.release();
    return AGX_OK;
}

int build_plan(agx_ntt_plan** out, uint32_t n, uint32_t num_primes, const uint64_t* moduli, const uint64_t* psi,
               const uint64_t* tw, const uint64_t* pre, const uint64_t* itw, const uint64_t* ipre) {
    plan_image img;
    prepare_plan_image(img, n, num_primes, moduli, psi, tw, pre, itw, ipre);
    return instantiate_plan(out, img);
}

}  // namespace agx

namespace {

uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }      // what operands.hpp takes
bool aligned8(const void* p) { return (addr(p) & 7u) == 0; }      // uint64_t data
bool batch_fits_grid(const agx_ntt_plan* plan, uint64_t batch) { return batch <= (0x7fffffffull >> (plan->log_n > 14 ? plan->log_n - 14 : 0)); }      // grid.x limit (the radix-2 kernels split n = 32768 in two blocks)

// The dense [prime][batch][n] layout of a plan, for the checks and the launches alike.  Nothing is multiplied for a batch past the grid
// limit, which check_frames refuses before it looks at a stride: batch * n stays below 2^46.
frame_layout dense(const agx_ntt_plan* plan, uint64_t batch) { return frame_layout{batch, batch_fits_grid(plan, batch) ? (int64_t)(batch * plan->n) : 0, (int64_t)plan->n}; }
uint64_t dense_words(const agx_ntt_plan* plan, uint64_t batch) { return plan->num_primes * batch * plan->n; }      // of a bounded batch: < 2^62

// Frame-set rule: the plan's frames in layout fl at `base`.  Batch first, then layout_fits: nothing after them can overflow (operands.hpp).
int check_frames(const agx_ntt_plan* plan, const void* base, const frame_layout& fl) {
    if (!base) return AGX_ERR_NULL_POINTER;
    if (!aligned8(base) || !batch_fits_grid(plan, fl.batch)) return AGX_ERR_BAD_ARGUMENT;
    if (fl.batch > 1 && fl.poly_stride < (int64_t)plan->n) return AGX_ERR_BAD_ARGUMENT;   // frames would overlap
    if (!layout_fits(plan->n, plan->num_primes, fl.batch, fl.prime_stride, fl.poly_stride)) return AGX_ERR_BAD_ARGUMENT;   // a negative stride, or an extent past 2^60 words
    if (self_overlap(plan->n, plan->num_primes, fl.batch, fl.prime_stride, fl.poly_stride)) return AGX_ERR_BAD_ARGUMENT;   // (p, b) and (p', b') share words
    return AGX_OK;
}

// Pair rule: a second set in the layout of the checked set at `base` is that set itself (in place) or touches none of its frames.
int check_pair(const agx_ntt_plan* plan, const void* base, const void* other, const frame_layout& fl) {
    if (!other) return AGX_ERR_NULL_POINTER;
    if (!aligned8(other)) return AGX_ERR_BAD_ARGUMENT;
    return partial_overlap(addr(base), addr(other), plan->n, plan->num_primes, fl.batch, fl.prime_stride, fl.poly_stride) ? AGX_ERR_BAD_ARGUMENT : AGX_OK;
}

static int plan_set_variant_impl(agx_ntt_plan* plan, int variant) {
    if (!plan) return AGX_ERR_NULL_POINTER;
    int config_id = -1;
    if (variant >= AGX_VARIANT_REGBLOCK_BASE) {
        config_id = variant - AGX_VARIANT_REGBLOCK_BASE;
        variant = AGX_VARIANT_REGBLOCK;
    }
    if (variant != AGX_VARIANT_AUTO && variant != AGX_VARIANT_LDS_RADIX2 && variant != AGX_VARIANT_REGBLOCK) return AGX_ERR_BAD_ARGUMENT;
    if (variant != AGX_VARIANT_LDS_RADIX2) {
        rb_selection sel = regblock_select(plan->n, config_id, plan->arith_level, plan->narrow_level);
        if (!sel.main) {
            if (variant == AGX_VARIANT_REGBLOCK) return AGX_ERR_BAD_SIZE;
            sel.main = plan->main.entry;      // AUTO where the registry has nothing for this plan: it keeps what it runs
        }
        if (sel.main != plan->main.entry) {
            // The new entry's tables are built first, from the natural-index tables read back (a plan keeps no host copies); any failure
            // up to here leaves the plan as it was.  The device finishes with the old tables before the swap releases them.
            host_pass_tables host{sel.main, {}, {}};
            std::vector<ulonglong2> pairs((size_t)plan->num_primes * plan->n);
            AGX_HIP(hipMemcpy(pairs.data(), plan->d_tw, pairs.size() * sizeof(ulonglong2), hipMemcpyDeviceToHost));
            host.fwd = build_pass_table(sel.main, pairs, plan->moduli, plan->n);
            if (plan->d_itw) {
                AGX_HIP(hipMemcpy(pairs.data(), plan->d_itw, pairs.size() * sizeof(ulonglong2), hipMemcpyDeviceToHost));
                host.inv = build_pass_table(sel.main, pairs, plan->moduli, plan->n);
            }
            pass_tables fresh;
            if (int rc = upload_pass_tables(fresh, host)) return rc;
            AGX_HIP(hipDeviceSynchronize());
            plan->main = std::move(fresh);
        }
        plan->chosen = sel;
        plan->explicit_id = config_id >= 0;
    }
    plan->variant = variant;
    resolve_routes(plan);
    return AGX_OK;
}

}  // namespace

extern "C" {

const char* agx_ntt_strerror(int status) {
    switch (status) {
        case AGX_OK: return "success";
        case AGX_ERR_NULL_POINTER: return "required pointer argument is NULL";
        case AGX_ERR_BAD_SIZE: return "n must be a power of two in [2, 32768]";
        case AGX_ERR_BAD_MODULUS: return "modulus must be an odd prime < 2^62 with q = 1 (mod 2n)";
        case AGX_ERR_BAD_ROOT: return "psi is not a primitive 2n-th root of unity mod q";
        case AGX_ERR_BAD_ARGUMENT: return "invalid argument";
        case AGX_ERR_NO_DEVICE: return "no HIP device available";
        case AGX_ERR_HIP: return "HIP runtime error (see agx_ntt_last_hip_error)";
        case AGX_ERR_ALLOC: return "allocation failed";
        case AGX_ERR_NO_INVERSE: return "plan has no inverse tables";
    }
    return "unknown status";
}

int agx_ntt_last_hip_error(void) { return g_last_hip_error; }

int agx_ntt_device_count(int* count) {
    if (!count) return AGX_ERR_NULL_POINTER;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return AGX_OK;
}

#ifdef AGX_DIAG
// lib/libagxntt_diag.so only (tools/agx_ntt_diag.h): where the registry's trace kernel writes its phase stamps
int agx_ntt_debug_set_trace_buffer(void* d_buf, uint64_t bytes) {
    if (!d_buf && bytes) return AGX_ERR_NULL_POINTER;
    AGX_HIP(agx::regblock_set_trace(static_cast<uint64_t*>(d_buf), bytes / 128));
    return AGX_OK;
}
#endif

int agx_ntt_plan_create(agx_ntt_plan** plan, uint32_t n, uint32_t num_primes, const uint64_t* moduli,
                        const uint64_t* twiddles, const uint64_t* precons,
                        const uint64_t* inv_twiddles, const uint64_t* inv_precons) {
    if (!plan) return AGX_ERR_NULL_POINTER;
    *plan = nullptr;
    if (int rc = check_create_args(n, num_primes, moduli, twiddles, precons, inv_twiddles, inv_precons)) return rc;
    return guarded([&] { return build_plan(plan, n, num_primes, moduli, nullptr, twiddles, precons, inv_twiddles, inv_precons); });
}

int agx_ntt_plan_create_auto(agx_ntt_plan** plan, uint32_t n, uint32_t num_primes, const uint64_t* moduli, const uint64_t* psi) {
    if (!plan || !moduli) return AGX_ERR_NULL_POINTER;
    *plan = nullptr;
    if (int rc = check_shape(n, num_primes)) return rc;
    return guarded([&]() -> int {
        plan_image img;
        if (int rc = prepare_auto_image(img, n, num_primes, moduli, psi)) return rc;
        return instantiate_plan(plan, img);
    });
}

int agx_ntt_plan_destroy(agx_ntt_plan* plan) {
    free_plan(plan);
    return AGX_OK;
}

int agx_ntt_plan_set_variant(agx_ntt_plan* plan, int variant) {
    return guarded([&] { return plan_set_variant_impl(plan, variant); });
}

int agx_ntt_plan_info(const agx_ntt_plan* plan, uint32_t* n, uint32_t* num_primes, int* device, int* has_inverse) {
    if (!plan) return AGX_ERR_NULL_POINTER;
    if (n) *n = plan->n;
    if (num_primes) *num_primes = plan->num_primes;
    if (device) *device = plan->device;
    if (has_inverse) *has_inverse = plan->has_inverse ? 1 : 0;
    return AGX_OK;
}

int agx_ntt_plan_forward_kernel(const agx_ntt_plan* plan, uint64_t batch, int* registry_id) {
    if (!plan || !registry_id) return AGX_ERR_NULL_POINTER;
    const rb_entry* e = forward_route(plan, batch).rb;
    *registry_id = e ? e->id : -1;
    return AGX_OK;
}

int agx_ntt_plan_get_modulus(const agx_ntt_plan* plan, uint32_t prime_index, uint64_t* q, uint64_t* psi) {
    if (!plan) return AGX_ERR_NULL_POINTER;
    if (prime_index >= plan->num_primes) return AGX_ERR_BAD_ARGUMENT;
    if (q) *q = plan->moduli[prime_index];
    if (psi) *psi = plan->psi[prime_index];
    return AGX_OK;
}

static int forward_common(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, const frame_layout& fl, void* stream) {
    if (!plan || !d_in || !d_out) return AGX_ERR_NULL_POINTER;
    int rc = check_plan(plan);
    if (rc || (rc = check_frames(plan, d_in, fl)) || (rc = check_pair(plan, d_in, d_out, fl))) return rc;      // out may BE in, never straddle it
    if (fl.batch == 0) return AGX_OK;
    const route& r = forward_route(plan, fl.batch);
    hipStream_t s = static_cast<hipStream_t>(stream);
    AGX_HIP(r.rb ? r.rb->launch(r, d_in, d_out, fl, s) : launch_forward_radix2(r, d_in, d_out, fl, s));
    return AGX_OK;
}

int agx_ntt_forward_strided(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, int64_t prime_stride, int64_t poly_stride, void* stream) {
    return forward_common(plan, d_in, d_out, frame_layout{batch, prime_stride, poly_stride}, stream);
}

int agx_ntt_inverse_strided(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, int64_t prime_stride, int64_t poly_stride, void* stream) {
    if (!plan || !d_in || !d_out) return AGX_ERR_NULL_POINTER;
    const frame_layout fl{batch, prime_stride, poly_stride};
    int rc = check_plan(plan);
    if (rc || (rc = check_frames(plan, d_in, fl)) || (rc = check_pair(plan, d_in, d_out, fl))) return rc;
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    const route& r = plan->routes.inverse;
    hipStream_t s = static_cast<hipStream_t>(stream);
    AGX_HIP(r.rb ? r.rb->launch_inv(r, d_in, nullptr, d_out, fl, s) : launch_inverse_radix2(r, d_in, d_out, fl, s));
    return AGX_OK;
}

int agx_ntt_forward(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, void* stream) {
    if (!plan) return AGX_ERR_NULL_POINTER;
    return forward_common(plan, d_in, d_out, dense(plan, batch), stream);
}

int agx_ntt_forward_lazy(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, void* stream) {
    if (!plan) return AGX_ERR_NULL_POINTER;
    frame_layout fl = dense(plan, batch);
    fl.lazy_out = true;
    return forward_common(plan, d_in, d_out, fl, stream);
}

int agx_ntt_inverse(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, void* stream) {
    if (!plan) return AGX_ERR_NULL_POINTER;
    const frame_layout fl = dense(plan, batch);
    return agx_ntt_inverse_strided(plan, d_in, d_out, batch, fl.prime_stride, fl.poly_stride, stream);
}

int agx_ntt_pointwise(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, void* stream) {
    if (!plan || !d_a || !d_b || !d_c) return AGX_ERR_NULL_POINTER;
    const frame_layout fl = dense(plan, batch);
    int rc = check_plan(plan);
    if (rc || (rc = check_frames(plan, d_c, fl)) || (rc = check_pair(plan, d_c, d_a, fl)) || (rc = check_pair(plan, d_c, d_b, fl))) return rc;
    if (batch == 0) return AGX_OK;
    AGX_HIP(launch_pointwise(plan->routes.forward, d_a, d_b, d_c, batch, static_cast<hipStream_t>(stream)));
    return AGX_OK;
}

int agx_ntt_polymul(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c,
                    uint64_t* d_scratch, uint64_t batch, void* stream) {
    if (!plan || !d_a || !d_b || !d_c) return AGX_ERR_NULL_POINTER;
    const frame_layout fl = dense(plan, batch);
    int rc = check_plan(plan);
    if (rc || (rc = check_frames(plan, d_c, fl)) || (rc = check_pair(plan, d_c, d_a, fl)) || (rc = check_pair(plan, d_c, d_b, fl))) return rc;      // c may BE a or b, never straddle them
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const route& r = plan->routes.polymul; r.rb) {
        // one kernel: both forward transforms, the product and the inverse stay on chip (24n bytes of HBM traffic);
        // every workgroup reads its a and b frames completely before it writes c, so c may alias either
        AGX_HIP(r.rb->launch_mul(r, d_a, d_b, d_c, fl, s));
        return AGX_OK;
    }
    if (!d_scratch) return AGX_ERR_NULL_POINTER;
    const uint64_t words = dense_words(plan, batch);
    auto scratch_touches = [&](const uint64_t* p) { return ranges_touch(addr(d_scratch), words, addr(p), words); };
    if (scratch_touches(d_a) || scratch_touches(d_b) || scratch_touches(d_c)) return AGX_ERR_BAD_ARGUMENT;      // not anywhere
    // scratch <- NTT(a); c <- NTT(b) (a is dead by now, so c may alias it); c <- INTT(c o scratch).
    // With the register-blocked inverse the product is taken while it loads (no pointwise pass) and
    // the forward results may stay lazily reduced.
    if (const route& r = plan->routes.inverse; r.rb) {
        if ((rc = agx_ntt_forward_lazy(plan, d_a, d_scratch, batch, stream))) return rc;
        if ((rc = agx_ntt_forward_lazy(plan, d_b, d_c, batch, stream))) return rc;
        AGX_HIP(r.rb->launch_inv(r, d_c, d_scratch, d_c, fl, s));
        return AGX_OK;
    }
    if ((rc = agx_ntt_forward(plan, d_a, d_scratch, batch, stream))) return rc;
    if ((rc = agx_ntt_forward(plan, d_b, d_c, batch, stream))) return rc;
    if ((rc = agx_ntt_pointwise(plan, d_c, d_scratch, d_c, batch, stream))) return rc;
    return agx_ntt_inverse(plan, d_c, d_c, batch, stream);
}

int agx_ntt_polymul_ntt(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_bhat, uint64_t* d_c,
                        uint64_t batch, uint64_t bhat_batch, void* stream) {
    if (!plan || !d_a || !d_bhat || !d_c) return AGX_ERR_NULL_POINTER;
    const frame_layout fl = dense(plan, batch);
    int rc = check_plan(plan);
    if (rc || (rc = check_frames(plan, d_a, fl)) || (rc = check_pair(plan, d_a, d_c, fl))) return rc;      // c may BE a, never straddle it
    if (bhat_batch != batch && bhat_batch != 1) return AGX_ERR_BAD_ARGUMENT;
    if (!aligned8(d_bhat)) return AGX_ERR_BAD_ARGUMENT;
    // c's [prime][batch][n] must not touch bhat's [prime][bhat_batch][n] anywhere: every workgroup of a prime reads bhat while others already write c
    if (ranges_touch(addr(d_c), dense_words(plan, batch), addr(d_bhat), dense_words(plan, bhat_batch))) return AGX_ERR_BAD_ARGUMENT;
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    const int64_t n = fl.poly_stride, bhat_prime_stride = (int64_t)bhat_batch * n, bhat_poly_stride = bhat_batch == 1 ? 0 : n;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const route& r = plan->routes.polymul_ntt; r.rb) {
        // one kernel: the forward transform, the product with bhat as it streams in and the inverse stay on chip
        AGX_HIP(r.rb->launch_mulhat(r, d_a, d_bhat, d_c, fl, bhat_prime_stride, bhat_poly_stride, s));
        return AGX_OK;
    }
    // generic path, no scratch: c <- NTT(a) (lazy: the product reduces its operands); c <- c o bhat in place; c <- INTT(c)
    if ((rc = agx_ntt_forward_lazy(plan, d_a, d_c, batch, stream))) return rc;
    AGX_HIP(launch_pointwise_bhat(plan->routes.forward, d_c, d_bhat, batch, bhat_prime_stride, bhat_poly_stride, s));
    return agx_ntt_inverse(plan, d_c, d_c, batch, stream);
}

int agx_ntt_rescale(const agx_ntt_plan* plan, const uint64_t* d_x, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, int mode, void* stream) {
    if (!plan || !d_x || !d_out || !d_scratch) return AGX_ERR_NULL_POINTER;
    const uint32_t P = plan->num_primes;
    if (P < 2 || (mode != AGX_RESCALE_FLOOR && mode != AGX_RESCALE_ROUND)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);
    int rc = check_plan(plan);
    if (rc || (rc = check_frames(plan, d_x, fl))) return rc;      // x: all P slabs
    if (!aligned8(d_out) || !aligned8(d_scratch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t slab = (uint64_t)fl.prime_stride, head = (P - 1) * slab;
    const uintptr_t x = addr(d_x), x_last = x + 8 * head, out = addr(d_out), scratch = addr(d_scratch);      // dense sets, one range each: x is P slabs, out P-1, the scratch one
    if (out != x && ranges_touch(out, head, x, head + slab)) return AGX_ERR_BAD_ARGUMENT;      // out IS slabs 0 .. P-2 of x (in place) or touches nothing of x, the last slab included: the first launch reads it
    if (ranges_touch(scratch, slab, out, head) || ranges_touch(scratch, slab, x, head)) return AGX_ERR_BAD_ARGUMENT;      // the scratch never touches out or slabs 0 .. P-2 of x: P-1 workgroups per frame read it while others already write
    if (scratch != x_last && ranges_touch(scratch, slab, x_last, slab)) return AGX_ERR_BAD_ARGUMENT;      // the scratch IS the last slab of x (the caller gives that slab up) or does not touch it
    if (!plan->rescale_legal) return AGX_ERR_BAD_MODULUS;      // some q_i shares a factor with (distinct primes: equals) the last modulus
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    const bool round = mode == AGX_RESCALE_ROUND;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // scratch <- INTT_L(x_L), coefficients in [0, q_L): the plan's inverse on the view of prime P-1
    const route last = prime_range(plan->routes.inverse, P - 1, P);
    auto inverse_on = [&](const route& r, const uint64_t* in, uint64_t* out_) {
        return r.rb ? r.rb->launch_inv(r, in, nullptr, out_, fl, s) : launch_inverse_radix2(r, in, out_, fl, s);
    };
    if (const route& r = plan->routes.rescale; r.rb) {
        // two launches: the lift, the forward transform and (x_i - .) q_L^-1 stay on chip; a wave reads its words of x_i before it writes them
        AGX_HIP(inverse_on(last, d_x + head, d_scratch));
        AGX_HIP(r.rb->launch_rescale(prime_range(r, 0, P - 1), d_x, d_scratch, d_out, fl, round, s));
        return AGX_OK;
    }
    // generic route, no more scratch: out <- INTT(x_0 .. x_{P-2}); scratch <- INTT_L(x_L); out <- (out - lift(scratch)) q_L^-1 in the
    // coefficient domain; out <- NTT(out)
    AGX_HIP(inverse_on(prime_range(plan->routes.inverse, 0, P - 1), d_x, d_out));
    AGX_HIP(inverse_on(last, d_x + head, d_scratch));
    const route head_route = prime_range(forward_route(plan, batch), 0, P - 1);
    AGX_HIP(launch_rescale_coeff(head_route, d_out, d_scratch, batch, round, s));
    AGX_HIP(head_route.rb ? head_route.rb->launch(head_route, d_out, d_out, fl, s) : launch_forward_radix2(head_route, d_out, d_out, fl, s));
    return AGX_OK;
}

int agx_ntt_automorphism(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t galois_elt, int form, void* stream) {
    if (!plan || !d_in || !d_out) return AGX_ERR_NULL_POINTER;
    int rc = check_plan(plan);
    if (rc || (rc = check_frames(plan, d_in, dense(plan, batch)))) return rc;
    if (!aligned8(d_out)) return AGX_ERR_BAD_ARGUMENT;
    if (!(galois_elt & 1u) || galois_elt >= 2u * plan->n || (form != AGX_FORM_COEFF && form != AGX_FORM_NTT)) return AGX_ERR_BAD_ARGUMENT;
    // out of place only, equal pointers included: a frame is permuted across its whole length and workgroups run in any order
    if (d_out == d_in || ranges_touch(addr(d_in), dense_words(plan, batch), addr(d_out), dense_words(plan, batch))) return AGX_ERR_BAD_ARGUMENT;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const route& r = plan->routes.forward;      // the per-prime constants only: no table, no plan state
    AGX_HIP(form == AGX_FORM_NTT ? launch_automorphism_ntt(r, d_in, d_out, batch, galois_elt, s) : launch_automorphism_coeff(r, d_in, d_out, batch, galois_elt, s));
    return AGX_OK;
}

int agx_ntt_basis_create(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count) {
    if (!basis) return AGX_ERR_NULL_POINTER;
    *basis = nullptr;
    if (!plan) return AGX_ERR_NULL_POINTER;
    const uint32_t P = plan->num_primes;
    auto in_plan = [&](uint32_t first, uint32_t count) { return count >= 1 && count <= P && first <= P - count; };
    if (!in_plan(src_first, src_count) || !in_plan(dst_first, dst_count) || src_count > AGX_BASIS_MAX_SRC) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    return guarded([&]() -> int {
        const uint32_t S = src_count, T = dst_count;
        std::vector<uint64_t> dinv(S), dinv_p(S), mat((size_t)T * S), mat_p((size_t)T * S);
        // D_i must be invertible modulo q_i: two equal source moduli have no conversion
        if (!basis_constants(&plan->moduli[src_first], S, &plan->moduli[dst_first], T, dinv.data(), dinv_p.data(), mat.data(), mat_p.data())) return AGX_ERR_BAD_MODULUS;
        std::vector<ulonglong2> dinv_pairs(S), mat_pairs((size_t)T * S);
        for (size_t k = 0; k < dinv_pairs.size(); ++k) dinv_pairs[k] = make_ulonglong2(dinv[k], dinv_p[k]);
        for (size_t k = 0; k < mat_pairs.size(); ++k) mat_pairs[k] = make_ulonglong2(mat[k], mat_p[k]);
        std::unique_ptr<agx_ntt_basis> b(new (std::nothrow) agx_ntt_basis);
        if (!b) return AGX_ERR_ALLOC;
        b->plan = plan;
        b->src_first = src_first, b->src_count = S, b->dst_first = dst_first, b->dst_count = T;
        if (int rc = b->d_dinv.upload(dinv_pairs)) return rc;
        if (int rc = b->d_mat.upload(mat_pairs)) return rc;
        // agx_ntt_basis_mod_down: D^-1 mod q_j, and the source primes' constants with the inverse's last-stage factors scaled by D_i^-1 (the plan
        // keeps no host copy of its constants: the S entries are read back).  A target that is a source modulus leaves the basis good for extend.
        std::vector<prime_consts> sc(S);
        AGX_HIP(hipMemcpy(sc.data(), plan->d_consts.p + src_first, S * sizeof(prime_consts), hipMemcpyDeviceToHost));
        std::vector<uint64_t> n_inv(S), w1n(S), dall(T), dall_p(T), sn(S), sn_p(S), sw(S), sw_p(S);
        for (uint32_t i = 0; i < S; ++i) n_inv[i] = sc[i].n_inv, w1n[i] = sc[i].w1n;
        b->moddown_legal = moddown_constants(&plan->moduli[src_first], S, &plan->moduli[dst_first], T, dinv.data(), n_inv.data(), w1n.data(), dall.data(),
                                             dall_p.data(), sn.data(), sn_p.data(), sw.data(), sw_p.data());
        for (uint32_t i = 0; i < S; ++i) sc[i].n_inv = sn[i], sc[i].n_inv_p = sn_p[i], sc[i].w1n = sw[i], sc[i].w1n_p = sw_p[i];
        std::vector<ulonglong2> dall_pairs(T);
        for (uint32_t j = 0; j < T; ++j) dall_pairs[j] = make_ulonglong2(dall[j], dall_p[j]);
        if (int rc = b->d_dall.upload(dall_pairs)) return rc;
        if (int rc = b->d_src_consts.upload(sc)) return rc;
        *basis = b.release();
        return AGX_OK;
    });
}

int agx_ntt_basis_destroy(agx_ntt_basis* basis) {
    delete basis;      // the device memory goes with its owners
    return AGX_OK;
}

// Does an AGX_FORM_NTT call of this basis take the fused kernel?  The plan's entry must carry it, and the shape must be one at which it was measured
// ahead of the unfused pair (profiles/r08_basis_extend.md).  Every workgroup of a frame forms the y_i again -- 2 S Shoup products per output word
// beside the transform's log2(n) / 2 -- so the fused kernel's arithmetic grows with S while the pair's conversion stays bound by its traffic:
//   S = 1: fused at every size (0.83 ... 0.92 of the pair's time);
//   S = 2: fused (0.96 ... 0.99) except at n = 4096 and 16384, where it measured 1.02 and 1.01 of the pair;
//   S >= 3: the pair (S = 4, 8, 16 measured: the fused kernel takes 1.21 ... 1.49 of its time; S = 3 not measured, taken with them).
static bool extend_is_fused(const agx_ntt_basis* b) {
    const agx_ntt_plan* p = b->plan;
    if (!p->routes.extend.rb) return false;
    return b->src_count == 1 || (b->src_count == 2 && p->log_n != 12 && p->log_n != 14);
}

// kernel launches of one forward call of the plan: a registry entry is one launch whatever the batch (forward and forward_large alike: the second
// exists only beside a first with an entry), the radix-2 kernels say themselves how many they take
static int forward_launches(const agx_ntt_plan* p) { return forward_route(p, 1).rb ? 1 : forward_radix2_launches(p->log_n); }

int agx_ntt_basis_info(const agx_ntt_basis* basis, uint32_t* src_first, uint32_t* src_count, uint32_t* dst_first, uint32_t* dst_count, int* launches_ntt_form) {
    if (!basis) return AGX_ERR_NULL_POINTER;
    if (src_first) *src_first = basis->src_first;
    if (src_count) *src_count = basis->src_count;
    if (dst_first) *dst_first = basis->dst_first;
    if (dst_count) *dst_count = basis->dst_count;
    if (launches_ntt_form) *launches_ntt_form = extend_is_fused(basis) ? 1 : 1 + forward_launches(basis->plan);
    return AGX_OK;
}

int agx_ntt_basis_extend(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t batch, int out_form, void* stream) {
    if (!basis || !d_x || !d_out) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = basis->plan;
    if (out_form != AGX_FORM_COEFF && out_form != AGX_FORM_NTT) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    const uint32_t S = basis->src_count, T = basis->dst_count;
    if (!aligned8(d_x) || !aligned8(d_out) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);      // of x ([S][batch][n]) and of out ([T][batch][n]) alike
    if (!layout_fits(plan->n, S, batch, fl.prime_stride, fl.poly_stride) || !layout_fits(plan->n, T, batch, fl.prime_stride, fl.poly_stride)) return AGX_ERR_BAD_ARGUMENT;
    // out of place only: every workgroup of a frame reads all S source frames while others already write their targets
    if (ranges_touch(addr(d_x), S * batch * plan->n, addr(d_out), T * batch * plan->n)) return AGX_ERR_BAD_ARGUMENT;
    const basis_view bv{basis->d_dinv, basis->d_mat, basis->d_dall, basis->src_first, S, basis->dst_first, T};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const route& r = plan->routes.extend; out_form == AGX_FORM_NTT && extend_is_fused(basis)) {
        // one kernel: the conversion and the target prime's forward transform stay on chip; T workgroups per group of rb->ppb frames
        if ((uint64_t)T * ((batch + r.rb->ppb - 1) / r.rb->ppb) > 0x7fffffffull) return AGX_ERR_BAD_ARGUMENT;      // grid limit
        if (batch == 0) return AGX_OK;
        AGX_HIP(r.rb->launch_extend(r, bv, d_x, d_out, fl, s));
        return AGX_OK;
    }
    if (batch == 0) return AGX_OK;
    AGX_HIP(launch_basis_coeff(plan->routes.forward, bv, d_x, d_out, batch, s));
    if (out_form == AGX_FORM_NTT) {      // the plan's forward on the view of the target primes, in place
        const route fr = prime_range(forward_route(plan, batch), basis->dst_first, basis->dst_first + T);
        AGX_HIP(fr.rb ? fr.rb->launch(fr, d_out, d_out, fl, s) : launch_forward_radix2(fr, d_out, d_out, fl, s));
    }
    return AGX_OK;
}

// Does a mod_down call of this basis take the two-launch route?  The plan's entry must carry the fused kernel (n = 1024 ... 32768, some modulus
// >= 2^31, not AGX_VARIANT_LDS_RADIX2); resolved at the call, so agx_ntt_plan_set_variant between calls stays legal.
// It serves every source count: measured at S = 1, 2, 4, 8, 16 against the four-launch route on the same plan (profiles/r09_mod_down.md).
static bool moddown_is_fused(const agx_ntt_basis* b) {
#ifdef AGX_DIAG
    // lib/libagxntt_diag.so only: AGX_NTT_MOD_DOWN_GENERIC=1 in the environment, read at every call, sends the call down the four-launch route on the
    // same plan (tools/run_op.py --op moddown times the two routes side by side)
    if (const char* e = std::getenv("AGX_NTT_MOD_DOWN_GENERIC"); e && e[0] == '1') return false;
#endif
    return b->plan->routes.moddown.rb != nullptr;
}

static int inverse_launches(const agx_ntt_plan* p) { return p->routes.inverse.rb ? 1 : inverse_radix2_launches(p->log_n); }

int agx_ntt_basis_mod_down_info(const agx_ntt_basis* basis, int* launches) {
    if (!basis) return AGX_ERR_NULL_POINTER;
    // fused: the scaled inverse of the source slabs, then moddown_rb2; generic: both inverses, the coefficient-domain step, the forward
    if (launches) *launches = moddown_is_fused(basis) ? inverse_launches(basis->plan) + 1 : 2 * inverse_launches(basis->plan) + 1 + forward_launches(basis->plan);
    return AGX_OK;
}

int agx_ntt_basis_mod_down(const agx_ntt_basis* basis, const uint64_t* d_xq, const uint64_t* d_xp, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream) {
    if (!basis || !d_xq || !d_xp || !d_out || !d_scratch) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = basis->plan;
    if (int rc = check_plan(plan)) return rc;
    const uint32_t S = basis->src_count, T = basis->dst_count;
    if (!aligned8(d_xq) || !aligned8(d_xp) || !aligned8(d_out) || !aligned8(d_scratch) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);      // of xq and out ([T][batch][n]) and of xp and the scratch ([S][batch][n]) alike
    if (!layout_fits(plan->n, S, batch, fl.prime_stride, fl.poly_stride) || !layout_fits(plan->n, T, batch, fl.prime_stride, fl.poly_stride)) return AGX_ERR_BAD_ARGUMENT;
    const bool fused = moddown_is_fused(basis);
    const route& r = plan->routes.moddown;
    if (fused && (uint64_t)T * ((batch + r.rb->ppb - 1) / r.rb->ppb) > 0x7fffffffull) return AGX_ERR_BAD_ARGUMENT;      // grid limit: T workgroups per group of rb->ppb frames
    const uint64_t slab = (uint64_t)fl.prime_stride, qwords = T * slab, pwords = S * slab;      // dense sets, one range each
    const uintptr_t xq = addr(d_xq), xp = addr(d_xp), out = addr(d_out), scratch = addr(d_scratch);
    if (out != xq && ranges_touch(out, qwords, xq, qwords)) return AGX_ERR_BAD_ARGUMENT;      // out IS xq (in place) or touches nothing of it
    // out never touches xp or the scratch, the scratch never xq: T workgroups per frame read the scratch while others already write out
    if (ranges_touch(out, qwords, xp, pwords) || ranges_touch(out, qwords, scratch, pwords) || ranges_touch(scratch, pwords, xq, qwords)) return AGX_ERR_BAD_ARGUMENT;
    if (scratch != xp && ranges_touch(scratch, pwords, xp, pwords)) return AGX_ERR_BAD_ARGUMENT;      // the scratch IS xp (the caller gives those slabs up) or does not touch it
    if (!basis->moddown_legal) return AGX_ERR_BAD_MODULUS;      // some target modulus is a source modulus: D has no inverse there
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    const basis_view bv{basis->d_dinv, basis->d_mat, basis->d_dall, basis->src_first, S, basis->dst_first, T};
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto inverse_on = [&](const route& v, const uint64_t* in, uint64_t* out_) {
        return v.rb ? v.rb->launch_inv(v, in, nullptr, out_, fl, s) : launch_inverse_radix2(v, in, out_, fl, s);
    };
    // scratch <- y_i = INTT_i(xp_i) D_i^-1 mod q_i in [0, q_i): the plan's inverse on the view of the source primes, its last-stage constants the basis'
    route scaled = prime_range(plan->routes.inverse, basis->src_first, basis->src_first + S);
    scaled.consts = basis->d_src_consts;
    if (fused) {
        // two launches: the accumulation, the forward transform and (xq_j - .) D^-1 stay on chip; a wave reads its words of xq_j before it writes them
        AGX_HIP(inverse_on(scaled, d_xp, d_scratch));
        AGX_HIP(r.rb->launch_moddown(r, bv, d_xq, d_scratch, d_out, fl, s));
        return AGX_OK;
    }
    // generic route, no more scratch: out <- INTT(xq) on the target primes; scratch <- the y_i; out <- (out - sum_i y_i D_i) D^-1 in the coefficient
    // domain; out <- NTT(out) in place
    AGX_HIP(inverse_on(prime_range(plan->routes.inverse, basis->dst_first, basis->dst_first + T), d_xq, d_out));
    AGX_HIP(inverse_on(scaled, d_xp, d_scratch));
    AGX_HIP(launch_moddown_coeff(plan->routes.forward, bv, d_out, d_scratch, batch, s));
    const route fr = prime_range(forward_route(plan, batch), basis->dst_first, basis->dst_first + T);
    AGX_HIP(fr.rb ? fr.rb->launch(fr, d_out, d_out, fl, s) : launch_forward_radix2(fr, d_out, d_out, fl, s));
    return AGX_OK;
}

// agx_ntt_inner_product and agx_ntt_inner_product_galois: one statement of the rules, the Galois element's between the overlap rule and the device's
static int inner_product_call(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_bhat, uint64_t* d_c, uint64_t batch, uint64_t bhat_batch,
                              uint32_t terms, uint32_t outputs, uint32_t galois_elt, void* stream) {
    if (!plan || !d_a || !d_bhat || !d_c) return AGX_ERR_NULL_POINTER;
    if (terms == 0 || terms > AGX_INNER_MAX_TERMS || outputs == 0 || outputs > AGX_INNER_MAX_OUTPUTS || (bhat_batch != batch && bhat_batch != 1)) return AGX_ERR_BAD_ARGUMENT;
    if (!aligned8(d_a) || !aligned8(d_bhat) || !aligned8(d_c)) return AGX_ERR_BAD_ARGUMENT;
    if (!batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;      // from here on batch n < 2^46
    // every operand is one dense range of `slabs` x frames x n words: layout_fits forms slabs frames n in 128 bits (terms outputs P <= 32 65535 slabs)
    const uint32_t P = plan->num_primes, n = plan->n;
    auto fits = [&](uint32_t slabs, uint64_t frames) { return layout_fits(n, slabs, frames, (int64_t)(frames * n), (int64_t)n); };
    if (!fits(terms * P, batch) || !fits(terms * outputs * P, bhat_batch) || !fits(outputs * P, batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t slab = batch * n, a_words = terms * P * slab, b_words = (uint64_t)terms * outputs * P * bhat_batch * n, c_words = outputs * P * slab;      // each <= 2^60
    // out of place only, equal pointers included: c_o of a word is written once, but by a thread that other threads' reads of a and bhat do not wait for
    if (ranges_touch(addr(d_c), c_words, addr(d_a), a_words) || ranges_touch(addr(d_c), c_words, addr(d_bhat), b_words)) return AGX_ERR_BAD_ARGUMENT;
    if (!(galois_elt & 1u) || galois_elt >= 2u * n) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (batch == 0) return AGX_OK;
    AGX_HIP(launch_inner_product_galois(plan->routes.forward, inner_primes{P, P, 0}, d_a, d_bhat, d_c, batch, bhat_batch, terms, outputs, galois_elt, static_cast<hipStream_t>(stream)));
    return AGX_OK;
}

int agx_ntt_inner_product(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_bhat, uint64_t* d_c, uint64_t batch, uint64_t bhat_batch,
                          uint32_t terms, uint32_t outputs, void* stream) {
    return inner_product_call(plan, d_a, d_bhat, d_c, batch, bhat_batch, terms, outputs, 1, stream);      // g = 1 (n >= 2: legal on every plan): the un-gathered kernel
}

int agx_ntt_inner_product_galois(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_bhat, uint64_t* d_c, uint64_t batch, uint64_t bhat_batch,
                                 uint32_t terms, uint32_t outputs, uint32_t galois_elt, void* stream) {
    return inner_product_call(plan, d_a, d_bhat, d_c, batch, bhat_batch, terms, outputs, galois_elt, stream);
}

int agx_ntt_keyswitch_create(agx_ntt_keyswitch** ks, const agx_ntt_plan* plan, uint32_t q_count, uint32_t p_first, uint32_t p_count, uint32_t alpha) {
    if (!ks) return AGX_ERR_NULL_POINTER;
    *ks = nullptr;
    if (!plan) return AGX_ERR_NULL_POINTER;
    const keyswitch_shape shape{q_count, p_first, p_count, alpha};
    if (!keyswitch_shape_ok(shape, plan->num_primes)) return AGX_ERR_BAD_ARGUMENT;
    // two equal moduli among the active primes: some D_i or D_P has no inverse where ModUp or ModDown needs one
    const uint32_t A = shape.active();
    auto modulus = [&](uint32_t slot) { return plan->moduli[slot < q_count ? slot : p_first + (slot - q_count)]; };
    for (uint32_t i = 0; i < A; ++i)
        for (uint32_t j = i + 1; j < A; ++j)
            if (modulus(i) == modulus(j)) return AGX_ERR_BAD_MODULUS;
    if (int rc = check_plan(plan)) return rc;
    return guarded([&]() -> int {
        std::unique_ptr<agx_ntt_keyswitch> k(new (std::nothrow) agx_ntt_keyswitch);
        if (!k) return AGX_ERR_ALLOC;
        k->plan = plan, k->shape = shape;
        k->up.reserve(2 * shape.digits());
        auto add = [&](uint32_t sf, uint32_t sc, uint32_t df, uint32_t dc) {
            agx_ntt_basis* b = nullptr;
            const int rc = agx_ntt_basis_create(&b, plan, sf, sc, df, dc);
            if (rc == AGX_OK) k->up.push_back(b);      // capacity reserved: the handle owns b from here
            return rc;
        };
        for (uint32_t d = 0; d < shape.digits(); ++d) {
            uint32_t first, count;
            keyswitch_digit(shape, d, &first, &count);
            if (!shape.apart()) {
                if (int rc = add(first, count, 0, A)) return rc;
            } else {
                if (int rc = add(first, count, 0, q_count)) return rc;
                if (int rc = add(first, count, p_first, p_count)) return rc;
            }
        }
        if (int rc = agx_ntt_basis_create(&k->down, plan, p_first, p_count, 0, q_count)) return rc;
        *ks = k.release();
        return AGX_OK;
    });
}

int agx_ntt_keyswitch_destroy(agx_ntt_keyswitch* ks) {
    delete ks;      // the bases go with it
    return AGX_OK;
}

int agx_ntt_keyswitch_info(const agx_ntt_keyswitch* ks, uint32_t* q_count, uint32_t* p_first, uint32_t* p_count, uint32_t* alpha, uint32_t* digits, int* launches) {
    if (!ks) return AGX_ERR_NULL_POINTER;
    if (q_count) *q_count = ks->shape.q_count;
    if (p_first) *p_first = ks->shape.p_first;
    if (p_count) *p_count = ks->shape.p_count;
    if (alpha) *alpha = ks->shape.alpha;
    if (digits) *digits = ks->shape.digits();
    if (launches) {
        // the inverse on Q + what every ModUp basis reports + the inner product + two ModDown calls, each under the plan's current variant
        int extend[2 * kKeyswitchMaxDigits], down = 0;
        for (size_t i = 0; i < ks->up.size(); ++i) (void)agx_ntt_basis_info(ks->up[i], nullptr, nullptr, nullptr, nullptr, &extend[i]);
        (void)agx_ntt_basis_mod_down_info(ks->down, &down);
        *launches = keyswitch_launches(inverse_launches(ks->plan), extend, (uint32_t)ks->up.size(), down);
    }
    return AGX_OK;
}

int agx_ntt_keyswitch_scratch_words(const agx_ntt_keyswitch* ks, uint64_t batch, uint64_t* words) {
    if (!ks || !words) return AGX_ERR_NULL_POINTER;
    keyswitch_scratch part;
    if (!keyswitch_scratch_partition(ks->shape, ks->plan->n, batch, &part)) return AGX_ERR_BAD_ARGUMENT;
    *words = part.total;
    return AGX_OK;
}

int agx_ntt_keyswitch_hoisted_words(const agx_ntt_keyswitch* ks, uint64_t batch, uint64_t* ext_words, uint64_t* decompose_scratch_words, uint64_t* apply_scratch_words) {
    if (!ks) return AGX_ERR_NULL_POINTER;
    keyswitch_hoisted part;
    if (!keyswitch_hoisted_partition(ks->shape, ks->plan->n, batch, &part)) return AGX_ERR_BAD_ARGUMENT;
    if (ext_words) *ext_words = part.ext;
    if (decompose_scratch_words) *decompose_scratch_words = part.decompose_scratch;
    if (apply_scratch_words) *apply_scratch_words = part.apply_scratch;
    return AGX_OK;
}

int agx_ntt_keyswitch_hoisted_info(const agx_ntt_keyswitch* ks, int* launches_decompose, int* launches_apply_decomposed) {
    if (!ks) return AGX_ERR_NULL_POINTER;
    // the two halves of agx_ntt_keyswitch_info's sum, each under the plan's current variant
    if (launches_decompose) {
        int extend[2 * kKeyswitchMaxDigits];
        for (size_t i = 0; i < ks->up.size(); ++i) (void)agx_ntt_basis_info(ks->up[i], nullptr, nullptr, nullptr, nullptr, &extend[i]);
        *launches_decompose = keyswitch_launches_decompose(inverse_launches(ks->plan), extend, (uint32_t)ks->up.size());
    }
    if (launches_apply_decomposed) {
        int down = 0;
        (void)agx_ntt_basis_mod_down_info(ks->down, &down);
        *launches_apply_decomposed = keyswitch_launches_apply_decomposed(down);
    }
    return AGX_OK;
}

// Steps 1 and 2 of a key switch, every argument checked by the caller: coeff [Q][batch][n] <- INTT(chat), ext [digits][A][batch][n] <- ModUp of every digit
static int keyswitch_decompose_steps(const agx_ntt_keyswitch* ks, const uint64_t* d_chat, uint64_t* ext, uint64_t* coeff, uint64_t batch, void* stream) {
    const agx_ntt_plan* plan = ks->plan;
    const keyswitch_shape& k = ks->shape;
    const uint32_t Q = k.q_count, A = k.active(), digits = k.digits();
    const uint64_t slab = batch * plan->n;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (1) coeff_j <- INTT_j(chat_j) in [0, q_j): the plan's inverse on the view of primes [0, Q), as ModDown runs it on its sources: no second plan
    const frame_layout fl = dense(plan, batch);
    const route qr = prime_range(plan->routes.inverse, 0, Q);
    AGX_HIP(qr.rb ? qr.rb->launch_inv(qr, d_chat, nullptr, coeff, fl, s) : launch_inverse_radix2(qr, d_chat, coeff, fl, s));
    // (2) ext_d <- NTT_j(e_{d,j}) for every active j: agx_ntt_basis_extend of digit d's slabs of coeff, routes as that call chooses them.  A digit's
    // own slabs are transformed again (they come out as chat_j reduced); copying them instead was not measured, so it is not done.
    for (uint32_t d = 0, b = 0; d < digits; ++d) {
        const uint64_t* x = coeff + (uint64_t)d * k.alpha * slab;
        uint64_t* e = ext + (uint64_t)d * A * slab;
        if (int rc = agx_ntt_basis_extend(ks->up[b++], x, e, batch, AGX_FORM_NTT, stream)) return rc;
        if (k.apart())
            if (int rc = agx_ntt_basis_extend(ks->up[b++], x, e + Q * slab, batch, AGX_FORM_NTT, stream)) return rc;
    }
    return AGX_OK;
}

// Steps 3 and 4, every argument checked by the caller: acc [2][A][batch][n] <- sum_d pi_g(ext_d) o key_{d,o}, out [2][Q][batch][n] <- ModDown of each half
static int keyswitch_apply_steps(const agx_ntt_keyswitch* ks, const uint64_t* ext, const uint64_t* d_keyhat, uint64_t* d_out, uint64_t* acc, uint64_t batch,
                                 uint32_t galois_elt, void* stream) {
    const agx_ntt_plan* plan = ks->plan;
    const keyswitch_shape& k = ks->shape;
    const uint32_t Q = k.q_count, A = k.active();
    const uint64_t slab = batch * plan->n;
    // (3) acc_o <- sum_d pi_g(ext_d) o key_{d,o} over the active primes: one launch, the key broadcast over the batch; g = 1 is the un-gathered kernel
    AGX_HIP(launch_inner_product_galois(plan->routes.forward, inner_primes{A, Q, k.p_first - Q}, ext, d_keyhat, acc, batch, 1, k.digits(), 2, galois_elt,
                                        static_cast<hipStream_t>(stream)));
    // (4) out_o <- ModDown of acc_o, its special slabs given up as the scratch
    for (uint32_t o = 0; o < 2; ++o) {
        uint64_t* xq = acc + (uint64_t)o * A * slab;
        if (int rc = agx_ntt_basis_mod_down(ks->down, xq, xq + Q * slab, d_out + o * Q * slab, xq + Q * slab, batch, stream)) return rc;
    }
    return AGX_OK;
}

// the rules the two halves share, after the NULL rule and the 2^60 limits: alignment, the two grid limits, and no two of the call's `count` buffers touching
static bool keyswitch_buffers_ok(const agx_ntt_keyswitch* ks, uint64_t batch, const uintptr_t* base, const uint64_t* words, int count) {
    for (int i = 0; i < count; ++i)
        if (base[i] & 7u) return false;
    // batch past the grid limit; A workgroups per group of frames on the one-launch ModUp and the two-launch ModDown (at least one frame per workgroup)
    if (!batch_fits_grid(ks->plan, batch) || (uint64_t)ks->shape.active() * batch > 0x7fffffffull) return false;
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j)
            if (ranges_touch(base[i], words[i], base[j], words[j])) return false;
    return true;
}

int agx_ntt_keyswitch_decompose(const agx_ntt_keyswitch* ks, const uint64_t* d_chat, uint64_t* d_ext, uint64_t* d_scratch, uint64_t batch, void* stream) {
    if (!ks || !d_chat || !d_ext || !d_scratch) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = ks->plan;
    keyswitch_hoisted part;
    if (!keyswitch_hoisted_partition(ks->shape, plan->n, batch, &part)) return AGX_ERR_BAD_ARGUMENT;      // every extent below is one of its three
    const uintptr_t base[3] = {addr(d_chat), addr(d_ext), addr(d_scratch)};
    const uint64_t words[3] = {part.decompose_scratch, part.ext, part.decompose_scratch};
    if (!keyswitch_buffers_ok(ks, batch, base, words, 3)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    return keyswitch_decompose_steps(ks, d_chat, d_ext, d_scratch, batch, stream);
}

int agx_ntt_keyswitch_apply_decomposed(const agx_ntt_keyswitch* ks, const uint64_t* d_ext, const uint64_t* d_keyhat, uint64_t* d_out, uint64_t* d_scratch,
                                       uint64_t batch, uint32_t galois_elt, void* stream) {
    if (!ks || !d_ext || !d_keyhat || !d_out || !d_scratch) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = ks->plan;
    const keyswitch_shape& k = ks->shape;
    keyswitch_hoisted part;
    if (!keyswitch_hoisted_partition(k, plan->n, batch, &part)) return AGX_ERR_BAD_ARGUMENT;
    const uintptr_t base[4] = {addr(d_ext), addr(d_keyhat), addr(d_out), addr(d_scratch)};
    const uint64_t words[4] = {part.ext, (uint64_t)k.digits() * 2 * k.active() * plan->n, 2 * part.decompose_scratch, part.apply_scratch};
    if (!keyswitch_buffers_ok(ks, batch, base, words, 4)) return AGX_ERR_BAD_ARGUMENT;
    if (!(galois_elt & 1u) || galois_elt >= 2u * plan->n) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;      // ModDown runs the plan's inverse
    if (batch == 0) return AGX_OK;
    return keyswitch_apply_steps(ks, d_ext, d_keyhat, d_out, d_scratch, batch, galois_elt, stream);
}

int agx_ntt_keyswitch_apply(const agx_ntt_keyswitch* ks, const uint64_t* d_chat, const uint64_t* d_keyhat, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream) {
    if (!ks || !d_chat || !d_keyhat || !d_out || !d_scratch) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = ks->plan;
    const keyswitch_shape& k = ks->shape;
    const uint32_t Q = k.q_count, A = k.active(), digits = k.digits(), n = plan->n;
    if (!aligned8(d_chat) || !aligned8(d_keyhat) || !aligned8(d_out) || !aligned8(d_scratch)) return AGX_ERR_BAD_ARGUMENT;
    // batch past the grid limit; A workgroups per group of frames on the one-launch ModUp and the two-launch ModDown (at least one frame per workgroup)
    if (!batch_fits_grid(plan, batch) || (uint64_t)A * batch > 0x7fffffffull) return AGX_ERR_BAD_ARGUMENT;
    keyswitch_scratch part;
    if (!keyswitch_scratch_partition(k, n, batch, &part)) return AGX_ERR_BAD_ARGUMENT;      // every extent below is a part of the scratch's or smaller
    const uint64_t slab = batch * n, chat_words = Q * slab, out_words = 2 * chat_words, key_words = (uint64_t)digits * 2 * A * n;
    const uintptr_t base[4] = {addr(d_chat), addr(d_keyhat), addr(d_out), addr(d_scratch)};
    const uint64_t words[4] = {chat_words, key_words, out_words, part.total};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (ranges_touch(base[i], words[i], base[j], words[j])) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    // the two halves on the three parts of the one scratch, with g = 1: the un-gathered inner product
    if (int rc = keyswitch_decompose_steps(ks, d_chat, d_scratch + part.ext, d_scratch + part.coeff, batch, stream)) return rc;
    return keyswitch_apply_steps(ks, d_scratch + part.ext, d_keyhat, d_out, d_scratch + part.acc, batch, 1, stream);
}

int agx_ntt_fill_synthetic(const agx_ntt_plan* plan, uint64_t* d_out, uint64_t batch, uint64_t first_poly, uint64_t seed, void* stream) {
    if (!plan || !d_out) return AGX_ERR_NULL_POINTER;
    int rc = check_plan(plan);
    if (rc || (rc = check_frames(plan, d_out, dense(plan, batch)))) return rc;
    if (batch == 0) return AGX_OK;
    AGX_HIP(launch_fill(plan->routes.forward, d_out, batch, first_poly, seed, static_cast<hipStream_t>(stream)));
    return AGX_OK;
}

}  // extern "C"
