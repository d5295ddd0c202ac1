// agx_ntt.cpp -- the extern "C" boundary declared in include/agx_ntt.h: plans and the transform and product calls.
// Owns plan objects (device tables, the routes from a call to its kernel), their argument validation and the mapping of HIP errors to
// status codes.  The RNS calls composed of these live in agx_basis.cpp, agx_ring.cpp, agx_keyswitch.cpp and agx_boundary.cpp, the steps and rules all share in plan_internal.hpp; kernels in
// ntt_kernels.hip and the registry groups; number theory in host_math.cpp; host-resident frames in agx_host.cpp.
#include "../../include/agx_ntt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "host_math.hpp"
#include "plan_internal.hpp"
#include "q60c_class.hpp"
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
    generic.consts = p->d_consts, generic.tw = p->d_tw, generic.itw = p->d_itw, generic.rescale = p->d_rescale, generic.q60c_skip = p->q60c_skip;
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
    // within level 3: every c at or below the limit up to which the two-twiddle butterfly may reduce on every second stage only (modarith.hpp:
    // q60c_skip_bounds); one larger c, and the whole plan keeps the every-stage kernel
    img.q60c_skip = img.arith_level == 3 && q60c_skip_class(moduli, num_primes);
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
    p->has_inverse = img.has_inverse, p->arith_level = img.arith_level, p->narrow_level = img.narrow_level, p->q60c_skip = img.q60c_skip;
    p->chosen = img.chosen;
    p->rescale_legal = img.rescale_legal;
    p->ticket_streams.reserve(kTicketSlots);      // plan_ticket_for() runs inside unguarded launch calls: it must never allocate
    p->ticket_events.assign(kTicketSlots, nullptr);
    p->ticket_pending.assign(kTicketSlots, 0);
    p->moduli = img.moduli;
    p->psi = img.psi;
    p->consts = img.consts;
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
            // The new entry's tables are built first, from the natural-index tables read back (a plan keeps no host copy of its tables); any failure
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
    AGX_HIP(run_forward(forward_route(plan, fl.batch), d_in, d_out, fl, static_cast<hipStream_t>(stream)));
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
    AGX_HIP(run_inverse(plan->routes.inverse, d_in, nullptr, d_out, fl, static_cast<hipStream_t>(stream)));
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

// agx_ntt_forward_range and agx_ntt_inverse_range: the whole-plan calls' rules in their order on the dense frames of `count` primes, the ring calls' range
// rule right behind the NULL rule; then the plan's route for this batch viewed on the range, as the RNS calls run it
static int range_call(bool inverse, const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t first, uint32_t count, void* stream) {
    if (!plan || !d_in || !d_out) return AGX_ERR_NULL_POINTER;
    const uint32_t n = plan->n;
    if (!primes_in_plan(plan, first, count)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    const frame_layout fl = dense(plan, batch);
    if (!aligned8(d_in) || !batch_fits_grid(plan, batch) || !layout_fits(n, count, batch, fl.prime_stride, fl.poly_stride)) return AGX_ERR_BAD_ARGUMENT;
    if (!aligned8(d_out) || partial_overlap(addr(d_in), addr(d_out), n, count, batch, fl.prime_stride, fl.poly_stride)) return AGX_ERR_BAD_ARGUMENT;      // out may BE in, never straddle it
    if (inverse && !plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (inverse) AGX_HIP(run_inverse_on(plan, first, count, nullptr, d_in, d_out, batch, s));
    else AGX_HIP(run_forward_on(plan, first, count, d_in, d_out, batch, s));
    return AGX_OK;
}

int agx_ntt_forward_range(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t prime_first, uint32_t prime_count, void* stream) {
    return range_call(false, plan, d_in, d_out, batch, prime_first, prime_count, stream);
}

int agx_ntt_inverse_range(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t prime_first, uint32_t prime_count, void* stream) {
    return range_call(true, plan, d_in, d_out, batch, prime_first, prime_count, stream);
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
        AGX_HIP(run_inverse(r, d_c, d_scratch, d_c, fl, s));      // in2: legal here, r has an entry
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

int agx_ntt_automorphism(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t galois_elt, int form, void* stream) {
    if (!plan || !d_in || !d_out) return AGX_ERR_NULL_POINTER;
    int rc = check_plan(plan);
    if (rc || (rc = check_frames(plan, d_in, dense(plan, batch)))) return rc;
    if (!aligned8(d_out)) return AGX_ERR_BAD_ARGUMENT;
    if (!galois_ok(galois_elt, plan->n) || !form_ok(form)) return AGX_ERR_BAD_ARGUMENT;
    // out of place only, equal pointers included: a frame is permuted across its whole length and workgroups run in any order
    if (d_out == d_in || ranges_touch(addr(d_in), dense_words(plan, batch), addr(d_out), dense_words(plan, batch))) return AGX_ERR_BAD_ARGUMENT;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const route& r = plan->routes.forward;      // the per-prime constants only: no table, no plan state
    AGX_HIP(form == AGX_FORM_NTT ? launch_automorphism_ntt(r, d_in, d_out, batch, galois_elt, s) : launch_automorphism_coeff(r, d_in, d_out, batch, galois_elt, s));
    return AGX_OK;
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
