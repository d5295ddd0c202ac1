// plan_internal.hpp -- what agx_ntt.cpp (plans, transform and product calls), the units of the RNS calls composed of them (agx_basis.cpp, agx_ring.cpp,
// agx_keyswitch.cpp, agx_boundary.cpp) and agx_group.cpp (multi-device groups) share.  Host only: no device unit includes it.  Not installed; the public surface is include/agx_ntt.h.
#pragma once
#include "../../include/agx_ntt.h"

#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#include "host_math.hpp"
#include "keyswitch_layout.hpp"
#include "operands.hpp"
#include "rb_registry.hpp"

constexpr int kMaxDevices = 64;          // size of every per-device table (kernel attributes set once, staging pool, one-shot plans); devices past it work uncached
constexpr uint32_t kTicketSlots = 64;    // distinct streams of one plan that may run ticket-drawing kernels; further streams get the stateless kernels

namespace agx {

int hip_fail(hipError_t e);      // records the HIP error for agx_ntt_last_hip_error() and maps it to a status
int& last_hip_error_slot();      // this thread's agx_ntt_last_hip_error() value (a group copies its failing shard's into the caller's)

#define AGX_HIP(expr)                                    \
    do {                                                 \
        hipError_t e_ = (expr);                          \
        if (e_ != hipSuccess) return agx::hip_fail(e_);  \
    } while (0)

// device memory of a plan: move-only, freed with its owner
template <class T>
struct device_buf {
    T* p = nullptr;
    device_buf() = default;
    device_buf(device_buf&& o) noexcept : p(o.p) { o.p = nullptr; }
    device_buf& operator=(device_buf&& o) noexcept { return std::swap(p, o.p), *this; }      // the old memory goes with `o`
    ~device_buf() { if (p) (void)hipFree(p); }
    operator T*() const { return p; }
    int upload(const T* src, size_t count) {      // into an empty owner
        AGX_HIP(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
        AGX_HIP(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
        return AGX_OK;
    }
    int upload(const std::vector<T>& src) { return upload(src.data(), src.size()); }
};

// host_math.hpp knows no HIP type: a vector of its pairs goes to the device as the ulonglong2 the kernels read
static_assert(sizeof(shoup_pair) == sizeof(ulonglong2) && alignof(shoup_pair) == alignof(ulonglong2), "shoup_pair is uploaded as ulonglong2");
inline int upload_pairs(device_buf<ulonglong2>& to, const std::vector<shoup_pair>& pairs) { return to.upload(reinterpret_cast<const ulonglong2*>(pairs.data()), pairs.size()); }

// the pass tables of one registry entry for every prime of a plan ([P][entry->table_pairs] each), on the host and on the device
template <class Table>
struct pass_tables_of {
    const rb_entry* entry = nullptr;
    Table fwd, inv;      // from the forward tables; from the inverse tables (empty / null: the plan has none, or the entry is forward-only here)
};
using host_pass_tables = pass_tables_of<std::vector<ulonglong2>>;
using pass_tables = pass_tables_of<device_buf<ulonglong2>>;

// How a call finds its kernel: a route is a ready-made plan_view, its `rb` the registry entry that serves the call (null: the radix-2 /
// generic kernels).  One route per operation, filled by resolve_routes (agx_ntt.cpp) whenever the plan's state changes.
using route = plan_view;
struct plan_routes {
    route forward;
    route forward_large;      // forward launches of >= min_frames frames (batch x primes); rb null: none, `forward` serves every launch
    uint32_t min_frames = 0;
    route inverse;            // rb set: rb->launch_inv; else the radix-2 inverse
    route polymul;            // rb set: rb->launch_mul; else two forwards + `inverse` (product fused into its load when that has an entry)
    route polymul_ntt;        // rb set: rb->launch_mulhat; else forward + product in place + inverse
    route extend;             // rb set: rb->launch_extend (agx_ntt_basis_extend to NTT form in one launch); else launch_basis_coeff, then `forward` in place on the target primes
    route rescale;            // rb set: `inverse` on prime P-1, then rb->launch_rescale on primes 0 .. P-2; else inverse, coefficient-domain step, forward
    route moddown;            // rb set: `inverse` (scaled constants) on the source primes, then rb->launch_moddown; else two inverses, launch_moddown_coeff, forward
};

}  // namespace agx

struct agx_ntt_plan {
    uint32_t n = 0, log_n = 0, num_primes = 0;
    int device = -1;
    int variant = AGX_VARIANT_AUTO;
    bool explicit_id = false;     // the variant named a registry id: that entry serves every call (no large-launch companion)
    bool has_inverse = false;
    int arith_level = 0;     // 0 exact only; 1: every modulus <= 2^61 (8q-lazy legal); 2: <= 2^60 (16q-lazy legal); 3: every modulus 2^60 - c, 0 < c < 2^28
    int narrow_level = 0;    // 1: every modulus < 2^31, 2: < 2^30 -- the 32-bit kernels are legal (with arith_level >= 1: tables honour the contract)
    bool q60c_skip = false;  // arith_level 3 and every c <= kQ60cSkipMaxC: every route carries it (plan_view::q60c_skip), the n = 4096 forward companion (id 165) launches its skip-form kernel
    std::vector<uint64_t> moduli, psi;  // psi = 0 when the tables came from the caller
    std::vector<agx::prime_consts> consts;      // [P]: what d_consts holds (64 bytes per prime; the tables below stay device-only)
    agx::device_buf<agx::prime_consts> d_consts;
    agx::device_buf<agx::rescale_consts> d_rescale;      // [P-1]; null for one prime
    bool rescale_legal = false;      // P >= 2 and q_{P-1} invertible modulo every other modulus (distinct primes are); judged at the call
    agx::device_buf<ulonglong2> d_tw, d_itw;      // [P][n] {w,w'} natural index; d_itw null without inverse tables
    agx::rb_selection chosen;      // the registry's answer for the current variant (LDS_RADIX2 leaves it as it was)
    agx::pass_tables main;         // of chosen.main; replaced when set_variant changes the entry
    // Of the tuned default's large-launch forward entry (forward table only): built at creation and kept for the plan's life, also
    // across an explicit choice, so that AUTO / REGBLOCK find it again.  It serves calls only while chosen.forward_large names it.
    agx::pass_tables companion;
    agx::plan_routes routes;
    // {next frame, retired workgroups} pairs for the kernels that hand out frames dynamically (the inverse loop kernels of n >= 16384),
    // one pair per STREAM: launches on one stream run one after the other, and the last workgroup of a launch zeroes the
    // pair, so a stream's launches can share one; launches on different streams get different pairs.  Only a launcher that needs a
    // pair asks for one (plan_view::ticket).  When all kTicketSlots are taken, a new stream gets the slot of a stream whose latest ticket
    // launch has provably completed (its event has fired: the pair is idle and zero); if there is none, no pair: the stateless fixed-stride
    // kernels (slots used to be claimed for good, so a long-lived plan used with short-lived streams ended up on the slower form).
    agx::device_buf<uint32_t> d_ticket;
    mutable std::mutex ticket_mu;
    mutable std::vector<hipStream_t> ticket_streams;
    // slot i: an event recorded behind the stream's latest ticket launch (once it has completed the pair reads {0, 0} again: the last
    // workgroup out zeroes it), and whether a launch that took the slot has not recorded its event yet
    mutable std::vector<hipEvent_t> ticket_events;
    mutable std::vector<char> ticket_pending;
};

// agx_ntt_basis_extend: the constants of one (plan, source range, target range) on the plan's device, and nothing of the plan but a pointer --
// the kernels come from the plan's routes at every call, so agx_ntt_plan_set_variant between calls stays legal.  The plan outlives the basis.
// Made from a basis_image (host_math.hpp, whose fields say what each buffer holds) by one function of agx_basis.cpp, which also fills the two views, once:
// a call hands them to its kernel as they are.  The ranges live in `view`; m and the two k of the auxiliary forms in `aux` only.
struct agx_ntt_basis {
    const agx_ntt_plan* plan = nullptr;
    agx::device_buf<ulonglong2> d_dinv, d_mat;      // agx_ntt_basis_extend
    // agx_ntt_basis_mod_down
    agx::device_buf<ulonglong2> d_dall;
    bool moddown_legal = false;              // every D^-1 mod q_j exists (no target modulus is a source modulus); judged at the call
    // [S]: the plan's prime_consts of the source primes with n_inv, w1n and their quotients replaced by the image's sn, sw.  The plan's inverse on the
    // view of the source primes with `consts` pointing here writes y_i = INTT_i(x_i) t^-1 D_i^-1 mod q_i in [0,q_i): every inverse family reads its
    // last-stage constants from its view's consts, and the transform is linear.
    agx::device_buf<agx::prime_consts> d_src_consts;
    // The plaintext modulus t of agx_ntt_basis_create_plain (1: agx_ntt_basis_create) is a property of ModDown alone and lives in constants only:
    // d_src_consts carry t^-1 mod q_i as well, and ModDown reads a matrix of its own, so agx_ntt_basis_extend keeps d_mat.
    agx::device_buf<ulonglong2> d_down_mat;
    agx::device_buf<ulonglong2> d_round_src;      // AGX_RESCALE_ROUND (agx_ntt_basis_mod_down_mode); AGX_RESCALE_FLOOR never reads the two
    agx::device_buf<uint64_t> d_round_dst;
    agx::basis_view view;
    // agx_ntt_basis_create_aux only: the auxiliary prime m = the modulus of plan prime aux_prime, and the constants of agx_ntt_basis_extend_exact and
    // agx_ntt_basis_extend_mont.  The exact form reads d_dinv and d_mat as agx_ntt_basis_extend does.
    bool has_aux = false;
    uint32_t aux_prime = 0;
    agx::device_buf<ulonglong2> d_aux_row, d_aux_corr_exact, d_aux_mdinv, d_aux_mmat, d_aux_corr_mont;
    agx::aux_view aux;
    // agx_ntt_basis_create_quotient only (such a basis has an auxiliary prime): the constants of agx_ntt_basis_quotient.  The prime_consts of the TARGET
    // primes ([T]) and of the sources followed by m ([S + 1]) with the last-stage factors replaced as d_src_consts has them, by the image's quot_dn / quot_dw
    // and quot_sn / quot_sw: the plan's inverse on those views writes the y_i, the s_j and s_m of bfv_quotient_arith.hpp.  aux_follows: m is the plan prime
    // right behind the sources, so one inverse launch serves Bsk.
    bool has_quotient = false, aux_follows = false;
    uint64_t quot_t = 0;
    agx::device_buf<agx::prime_consts> d_quot_dst_consts, d_quot_src_consts;
    agx::device_buf<ulonglong2> d_quot_mat;      // [T][S + 1]
};

// agx_ntt_plain_*: the constants of one plaintext boundary (plan, Q, gamma, t) on the plan's device, and nothing of the plan but a pointer, as a basis: the
// plan outlives the handle, agx_ntt_plan_set_variant between calls stays legal.  Made from a plain_image (host_math.hpp, whose fields say what each buffer
// holds) by one function of agx_boundary.cpp, which also fills the view, once.  d_src_consts: the plan's prime_consts of the Q primes with the last-stage factors
// replaced by the image's sn, sw, as a basis' d_src_consts: the plan's inverse on the view of Q with `consts` pointing here writes the y_i of scale_down.
struct agx_ntt_plain {
    const agx_ntt_plan* plan = nullptr;
    uint32_t gamma_prime = 0;
    agx::device_buf<ulonglong2> d_up, d_one, d_row_t, d_row_g;
    agx::device_buf<agx::prime_consts> d_src_consts;
    agx::device_buf<uint64_t> d_q;                   // agx_ntt_plain_reduce: the moduli, Garner's constants (empty for one prime), the digit weights modulo t
    agx::device_buf<ulonglong2> d_tri, d_radix_t;
    agx::plain_view view;
};

// agx_ntt_batch_*: a batching handle (n, t) on the device it was made on.  It OWNS its one-prime plan under t (made by agx_ntt_plan_create_auto with the least
// root and inverse tables; agx_ntt_batch_plan lends it) and the two index tables of a batch_image (host_math.hpp); the view is filled once.
struct agx_ntt_batch {
    agx_ntt_plan* plan = nullptr;
    uint64_t psi = 0;
    agx::device_buf<uint32_t> d_slot_to_word, d_word_to_slot;
    agx::batch_view view;
    agx_ntt_batch() = default;
    agx_ntt_batch(const agx_ntt_batch&) = delete;
    agx_ntt_batch& operator=(const agx_ntt_batch&) = delete;
    ~agx_ntt_batch();      // agx_boundary.cpp: the plan goes with its owner
};

// agx_ntt_ckks_*: the tables of one CKKS boundary (plan, the primes [q_first, q_first + q_count)) on the plan's device, and nothing of the plan but a pointer,
// as a basis: the plan outlives the handle, agx_ntt_plan_set_variant between calls stays legal.  Made from a ckks_image (host_math.hpp, whose fields say what
// each buffer holds) by one function of agx_boundary.cpp, which also fills the view, once.
struct agx_ntt_ckks {
    const agx_ntt_plan* plan = nullptr;
    agx::device_buf<double2> d_tw;
    agx::device_buf<uint64_t> d_q;
    agx::device_buf<ulonglong2> d_tri, d_pow2;
    agx::ckks_view view;
};

// agx_ntt_keyswitch_*: the shape and the bases of one hybrid key switch, and nothing of the plan but a pointer (as a basis: the plan outlives the
// handle, agx_ntt_plan_set_variant between calls stays legal).  ModUp: one basis per digit with every active prime as a target when the special
// primes follow Q directly; two per digit, targets Q and then targets P, when they lie apart (a basis names one contiguous range).  One ModDown
// basis, sources the special primes, targets Q.
struct agx_ntt_keyswitch {
    const agx_ntt_plan* plan = nullptr;
    agx::keyswitch_shape shape;
    std::vector<agx_ntt_basis*> up;      // [digits] or [digits][2]
    agx_ntt_basis* down = nullptr;
    agx_ntt_keyswitch() = default;
    agx_ntt_keyswitch(const agx_ntt_keyswitch&) = delete;
    agx_ntt_keyswitch& operator=(const agx_ntt_keyswitch&) = delete;
    ~agx_ntt_keyswitch() {
        for (agx_ntt_basis* b : up) delete b;
        delete down;
    }
};

namespace agx {

// nothing may propagate across the C boundary: std::vector / std::thread can throw inside the entry points
template <class F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return AGX_ERR_ALLOC;
    } catch (const std::system_error&) {      // std::thread could not be created
        return AGX_ERR_ALLOC;
    } catch (...) {
        return AGX_ERR_BAD_ARGUMENT;
    }
}

// a std::thread that is always joined before it is destroyed (unwinding past a joinable std::thread calls std::terminate)
struct joining_thread {
    std::thread t;
    joining_thread() = default;
    template <class F>
    explicit joining_thread(F&& f) : t(std::forward<F>(f)) {}
    joining_thread(joining_thread&&) = default;
    joining_thread& operator=(joining_thread&& o) {
        join();
        t = std::move(o.t);
        return *this;
    }
    void join() {
        if (t.joinable()) t.join();
    }
    ~joining_thread() { join(); }
};

// Everything of a plan that does not depend on the device: validated levels, per-prime constants and the tables in the layouts the
// kernels read.  Built once on the host (a 128-bit divide per table entry), uploaded to as many devices as the caller has.
struct plan_image {
    uint32_t n = 0, log_n = 0, num_primes = 0;
    bool has_inverse = false;
    int arith_level = 0, narrow_level = 0;
    bool q60c_skip = false;      // arith_level 3 and every modulus 2^60 - c has c <= kQ60cSkipMaxC
    std::vector<uint64_t> moduli, psi;
    rb_selection chosen;
    std::vector<prime_consts> consts;
    std::vector<rescale_consts> rescale;      // [P-1] (agx_ntt_rescale); entries of moduli that share a factor with the last stay zero
    bool rescale_legal = false;
    std::vector<ulonglong2> tw_pairs, itw_pairs;
    std::vector<host_pass_tables> tables;      // one per distinct entry `chosen` names, the main entry first
};
// arguments as validated by agx_ntt_plan_create*: moduli legal for n, tables [num_primes][n]; psi / itw / ipre may be null
void prepare_plan_image(plan_image& img, uint32_t n, uint32_t num_primes, const uint64_t* moduli, const uint64_t* psi,
                        const uint64_t* tw, const uint64_t* pre, const uint64_t* itw, const uint64_t* ipre);
// the same for agx_ntt_{plan,group}_create_auto, from (moduli, psi or null: the least roots): judges primes and roots, generates the tables
int prepare_auto_image(plan_image& img, uint32_t n, uint32_t num_primes, const uint64_t* moduli, const uint64_t* psi);
// a plan on the CURRENT device from a prepared image
int instantiate_plan(agx_ntt_plan** out, const plan_image& img);
void free_plan(agx_ntt_plan* p);
// argument checks and the plan construction that agx_ntt_plan_create shares with the groups and the one-shot calls of agx_host.cpp
int check_size(uint32_t n);
int check_modulus(uint64_t q, uint32_t n);
int check_shape(uint32_t n, uint32_t num_primes);      // check_size, then 1 .. 65535 primes
int check_plan(const agx_ntt_plan* plan);               // the plan exists and the current device is its device
// of agx_ntt_{plan,group}_create (one-shot: one modulus, no inverse tables): the pointer rules, check_shape, check_modulus of every modulus
int check_create_args(uint32_t n, uint32_t num_primes, const uint64_t* moduli, const uint64_t* tw, const uint64_t* pre, const uint64_t* itw, const uint64_t* ipre);
int build_plan(agx_ntt_plan** out, uint32_t n, uint32_t num_primes, const uint64_t* moduli, const uint64_t* psi,
               const uint64_t* tw, const uint64_t* pre, const uint64_t* itw, const uint64_t* ipre);

// ---- what the entry points of agx_ntt.cpp and of the RNS units (agx_basis.cpp, agx_ring.cpp, agx_keyswitch.cpp, agx_boundary.cpp) share: each launch
// step, each frame rule and each argument rule once ----

// The plan's forward / inverse on the frames a route views: the route's registry entry, or the radix-2 kernels.  in2 != null (the product in * in2
// is transformed) only with an entry.
inline hipError_t run_forward(const route& r, const uint64_t* in, uint64_t* out, const frame_layout& fl, hipStream_t s) {
    return r.rb ? r.rb->launch(r, in, out, fl, s) : launch_forward_radix2(r, in, out, fl, s);
}
inline hipError_t run_inverse(const route& r, const uint64_t* in, const uint64_t* in2, uint64_t* out, const frame_layout& fl, hipStream_t s) {
    return r.rb ? r.rb->launch_inv(r, in, in2, out, fl, s) : launch_inverse_radix2(r, in, out, fl, s);
}

inline const route& forward_route(const agx_ntt_plan* p, uint64_t batch) {
    const plan_routes& r = p->routes;
    return r.forward_large.rb && batch * p->num_primes >= r.min_frames ? r.forward_large : r.forward;
}

// kernel launches of one forward / inverse call of the plan: a registry entry is one launch whatever the batch (forward and forward_large alike: the
// second exists only beside a first with an entry), the radix-2 kernels say themselves how many they take
inline int forward_launches(const agx_ntt_plan* p) { return forward_route(p, 1).rb ? 1 : forward_radix2_launches(p->log_n); }
inline int inverse_launches(const agx_ntt_plan* p) { return p->routes.inverse.rb ? 1 : inverse_radix2_launches(p->log_n); }

inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }      // what operands.hpp takes
inline bool aligned8(const void* p) { return (addr(p) & 7u) == 0; }      // uint64_t data
inline bool galois_ok(uint32_t g, uint32_t n) { return (g & 1u) && g < 2u * n; }      // a Galois element: odd, in [1, 2n)
inline bool batch_fits_grid(const agx_ntt_plan* plan, uint64_t batch) { return batch <= (0x7fffffffull >> (plan->log_n > 14 ? plan->log_n - 14 : 0)); }      // grid.x limit (the radix-2 kernels split n = 32768 in two blocks)
inline bool dense_fits(uint32_t n, uint32_t slabs, uint64_t frames) { return layout_fits(n, slabs, frames, (int64_t)(frames * n), (int64_t)n); }      // one dense range of slabs x frames x n words (formed in 128 bits)
// The argument rules every family states, each as the calls wrote it, negated: a range of at least one of the plan's primes (first + count is never formed),
// a form and a rounding mode of include/agx_ntt.h
inline bool primes_in_plan(const agx_ntt_plan* plan, uint32_t first, uint32_t count) { const uint32_t P = plan->num_primes; return !(count == 0 || count > P || first > P - count); }
inline bool form_ok(int form) { return !(form != AGX_FORM_COEFF && form != AGX_FORM_NTT); }
inline bool mode_ok(int mode) { return !(mode != AGX_RESCALE_FLOOR && mode != AGX_RESCALE_ROUND); }

// The dense [prime][batch][n] layout of a plan, for the checks and the launches alike.  Nothing is multiplied for a batch past the grid
// limit, which check_frames refuses before it looks at a stride: batch * n stays below 2^46.
inline frame_layout dense(const agx_ntt_plan* plan, uint64_t batch) { return frame_layout{batch, batch_fits_grid(plan, batch) ? (int64_t)(batch * plan->n) : 0, (int64_t)plan->n}; }
inline uint64_t dense_words(const agx_ntt_plan* plan, uint64_t batch) { return plan->num_primes * batch * plan->n; }      // of a bounded batch: < 2^62

// The plan's forward / inverse on the view of primes [first, first + count), dense frames: what every RNS call and agx_ntt_{forward,inverse}_range run.
// The forward takes the route forward_route chooses for this batch on the WHOLE plan (batch x the plan's primes against min_frames, not the range's).
// consts null: the plan's own constants; else a handle's scaled constants (scaled_consts below), already at the range's first prime as prime_range
// leaves the plan's: every inverse family reads its last-stage factors there.
inline hipError_t run_forward_on(const agx_ntt_plan* plan, uint32_t first, uint32_t count, const uint64_t* in, uint64_t* out, uint64_t batch, hipStream_t s) {
    return run_forward(prime_range(forward_route(plan, batch), first, first + count), in, out, dense(plan, batch), s);
}
inline hipError_t run_inverse_on(const agx_ntt_plan* plan, uint32_t first, uint32_t count, const prime_consts* consts, const uint64_t* in, uint64_t* out, uint64_t batch,
                                 hipStream_t s) {
    route r = prime_range(plan->routes.inverse, first, first + count);
    if (consts) r.consts = consts;
    return run_inverse(r, in, nullptr, out, dense(plan, batch), s);
}

// ---- what the handles made from a host image (bases, agx_boundary.cpp's) share ----

// The plan's prime_consts of primes [first, first + count) with the inverse's last-stage factors (n_inv, w1n and their quotients) replaced by sn, sw
// ([count] each): what run_inverse_on takes as `consts`
inline std::vector<prime_consts> scaled_consts(const agx_ntt_plan* plan, uint32_t first, uint32_t count, const shoup_pair* sn, const shoup_pair* sw) {
    std::vector<prime_consts> c(plan->consts.begin() + first, plan->consts.begin() + first + count);
    for (uint32_t i = 0; i < count; ++i) c[i].n_inv = sn[i].w, c[i].n_inv_p = sn[i].p, c[i].w1n = sw[i].w, c[i].w1n_p = sw[i].p;
    return c;
}

// the unscaled factors of the same range, as the image requests of host_math.hpp take them
inline void inverse_factors(const agx_ntt_plan* plan, uint32_t first, uint32_t count, std::vector<uint64_t>& n_inv, std::vector<uint64_t>& w1n) {
    n_inv.resize(count), w1n.resize(count);
    for (uint32_t i = 0; i < count; ++i) n_inv[i] = plan->consts[first + i].n_inv, w1n[i] = plan->consts[first + i].w1n;
}

// One upload of a handle's list: skipped once an earlier one has failed, so rc keeps the first failure and the list ends in one `if (rc) return rc;`.
// The order of the list is the allocation order on the device.
template <class T>
inline void upload_next(int& rc, device_buf<T>& to, const std::vector<T>& from) { if (rc == AGX_OK) rc = to.upload(from); }
inline void upload_next(int& rc, device_buf<ulonglong2>& to, const std::vector<shoup_pair>& pairs) { if (rc == AGX_OK) rc = upload_pairs(to, pairs); }

// Frame-set rule: the plan's frames in layout fl at `base`.  Batch first, then layout_fits: nothing after them can overflow (operands.hpp).
inline int check_frames(const agx_ntt_plan* plan, const void* base, const frame_layout& fl) {
    if (!base) return AGX_ERR_NULL_POINTER;
    if (!aligned8(base) || !batch_fits_grid(plan, fl.batch)) return AGX_ERR_BAD_ARGUMENT;
    if (fl.batch > 1 && fl.poly_stride < (int64_t)plan->n) return AGX_ERR_BAD_ARGUMENT;   // frames would overlap
    if (!layout_fits(plan->n, plan->num_primes, fl.batch, fl.prime_stride, fl.poly_stride)) return AGX_ERR_BAD_ARGUMENT;   // a negative stride, or an extent past 2^60 words
    if (self_overlap(plan->n, plan->num_primes, fl.batch, fl.prime_stride, fl.poly_stride)) return AGX_ERR_BAD_ARGUMENT;   // (p, b) and (p', b') share words
    return AGX_OK;
}

// Pair rule: a second set in the layout of the checked set at `base` is that set itself (in place) or touches none of its frames.
inline int check_pair(const agx_ntt_plan* plan, const void* base, const void* other, const frame_layout& fl) {
    if (!other) return AGX_ERR_NULL_POINTER;
    if (!aligned8(other)) return AGX_ERR_BAD_ARGUMENT;
    return partial_overlap(addr(base), addr(other), plan->n, plan->num_primes, fl.batch, fl.prime_stride, fl.poly_stride) ? AGX_ERR_BAD_ARGUMENT : AGX_OK;
}

// staging resources of the host-pointer pipeline (agx_host.cpp): three slots of {pinned in, pinned out, device} on three streams
constexpr size_t kStageChunkBytes = (size_t)32 << 20;
struct staging_set {
    static constexpr int kSlots = 3;
    uint64_t *pin_in[kSlots] = {}, *pin_out[kSlots] = {}, *dev[kSlots] = {};
    hipStream_t st[kSlots] = {};
    hipEvent_t done[kSlots] = {};
    size_t bytes = 0;
    hipError_t ensure(size_t want);
    void destroy();
};
// host frames through `plan` (one modulus) with upload, transform and download overlapped; `own` = staging resources the caller
// keeps for this purpose (a group's shard), or null: the per-device pool, or a temporary set when the pool is busy
int host_stream_pipeline(const agx_ntt_plan* plan, const uint64_t* in, const uint64_t* in2, uint64_t* out, uint64_t num_frames,
                         bool inverse, staging_set* own);

}  // namespace agx
