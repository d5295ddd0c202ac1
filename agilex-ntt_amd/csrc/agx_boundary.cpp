// agx_boundary.cpp -- the scheme boundaries, each a handle made from a host image (host_math.hpp): BFV's plaintext boundary agx_ntt_plain_* (create, destroy,
// info, scale_up, lift, scale_down, reduce), CKKS encoding agx_ntt_ckks_* (create, destroy, info, encode, decode, twiddle) and slot batching agx_ntt_batch_*
// (create, destroy, info, plan, encode, decode), whose handle owns its own one-prime plan.
#include <memory>

#include "host_math.hpp"
#include "plan_internal.hpp"

using namespace agx;

extern "C" {

// ---- agx_ntt_plain_*: BFV's plaintext boundary (include/agx_ntt.h has the contract, plain_arith.hpp the formulas) ----

// A plaintext boundary on the current device from its image: the buffers, then the view every call hands to its kernel
static int instantiate_plain(agx_ntt_plain** out, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count, uint32_t gamma_prime, uint64_t t, const plain_image& img) {
    std::unique_ptr<agx_ntt_plain> p(new (std::nothrow) agx_ntt_plain);
    if (!p) return AGX_ERR_ALLOC;
    p->plan = plan, p->gamma_prime = gamma_prime;
    int rc = AGX_OK;
    upload_next(rc, p->d_up, img.up), upload_next(rc, p->d_one, img.one), upload_next(rc, p->d_row_t, img.row_t), upload_next(rc, p->d_row_g, img.row_g);
    upload_next(rc, p->d_radix_t, img.radix_t);
    if (!img.tri.empty()) upload_next(rc, p->d_tri, img.tri);      // one prime has no Garner constant
    upload_next(rc, p->d_q, img.q);
    upload_next(rc, p->d_src_consts, scaled_consts(plan, q_first, q_count, img.sn.data(), img.sw.data()));
    if (rc) return rc;
    plain_view& v = p->view;
    v.q = p->d_q, v.tri = p->d_tri, v.radix_t = p->d_radix_t;
    v.up = p->d_up, v.one = p->d_one, v.row_t = p->d_row_t, v.row_g = p->d_row_g;
    v.t = t, v.h = img.h, v.one_p = img.one_t.p, v.d = img.d_t.w, v.dp = img.d_t.p;
    v.gamma = plan->moduli[gamma_prime], v.g = img.g_t.w, v.gp = img.g_t.p;
    v.q_first = q_first, v.q_count = q_count;
    *out = p.release();
    return AGX_OK;
}

// agx_ntt_plain_scale_down and agx_ntt_plain_reduce: one statement of their rules, agx_ntt_basis_quotient's in its order, up to the empty batch (the caller's)
static int plain_down_rules(const agx_ntt_plain* h, const uint64_t* d_x, const uint64_t* d_m, const uint64_t* d_scratch, uint64_t batch) {
    if (!h || !d_x || !d_m || !d_scratch) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = h->plan;
    if (int rc = check_plan(plan)) return rc;
    const uint32_t L = h->view.q_count;
    if (!aligned8(d_x) || !aligned8(d_m) || !aligned8(d_scratch) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);      // of x and the scratch ([L][batch][n]) and of m ([1][batch][n]) alike
    if (!dense_fits(plan->n, L, batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t slab = (uint64_t)fl.prime_stride;
    if (!scratch_buffers_ok(addr(d_x), L * slab, addr(d_scratch), addr(d_m), slab)) return AGX_ERR_BAD_ARGUMENT;      // the inverse may run in place
    return plan->has_inverse ? AGX_OK : AGX_ERR_NO_INVERSE;
}

// agx_ntt_plain_scale_up and _lift: one statement of the rules, in extend_call's order.  Out of place only: d_out's L slabs touch d_m nowhere.
static int plain_encode_call(const agx_ntt_plain* h, bool lift, const uint64_t* d_m, uint64_t* d_out, uint64_t batch, int out_form, void* stream) {
    if (!h || !d_m || !d_out) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = h->plan;
    if (!form_ok(out_form)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    const plain_view& cv = h->view;
    const uint32_t L = cv.q_count;
    if (!aligned8(d_m) || !aligned8(d_out) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    if (!dense_fits(plan->n, L, batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t slab = batch * plan->n;
    if (ranges_touch(addr(d_m), slab, addr(d_out), L * slab)) return AGX_ERR_BAD_ARGUMENT;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    AGX_HIP(launch_plain_encode(plan->routes.forward, cv, lift, d_m, d_out, batch, s));
    if (out_form == AGX_FORM_NTT) AGX_HIP(run_forward_on(plan, cv.q_first, L, d_out, d_out, batch, s));      // Q, in place
    return AGX_OK;
}

// The rules in their order, agx_ntt_basis_create_aux's: NULL; the range and gamma's place, a bad argument; the plan; two moduli of Q that share a factor, gamma
// sharing one with a modulus of Q, a bad modulus; t outside [2, 2^62), a bad argument; t sharing a factor with some q_i, then with gamma, a bad modulus.
int agx_ntt_plain_create(agx_ntt_plain** h, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count, uint32_t gamma_prime, uint64_t t) {
    if (!h) return AGX_ERR_NULL_POINTER;
    *h = nullptr;
    if (!plan) return AGX_ERR_NULL_POINTER;
    const uint32_t P = plan->num_primes;
    if (!primes_in_plan(plan, q_first, q_count) || q_count > AGX_BASIS_MAX_SRC) return AGX_ERR_BAD_ARGUMENT;
    if (gamma_prime >= P || (gamma_prime >= q_first && gamma_prime - q_first < q_count)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    return guarded([&]() -> int {
        std::vector<uint64_t> n_inv, w1n;
        inverse_factors(plan, q_first, q_count, n_inv, w1n);
        plain_image img;
        switch (prepare_plain_image(img, plain_request{&plan->moduli[q_first], q_count, n_inv.data(), w1n.data(), plan->moduli[gamma_prime], t})) {
            case plain_fault::none: return instantiate_plain(h, plan, q_first, q_count, gamma_prime, t, img);
            case plain_fault::t_range: return AGX_ERR_BAD_ARGUMENT;
            default: return AGX_ERR_BAD_MODULUS;
        }
    });
}

int agx_ntt_plain_destroy(agx_ntt_plain* h) {
    delete h;      // the device memory goes with its owners
    return AGX_OK;
}

int agx_ntt_plain_info(const agx_ntt_plain* h, uint32_t* q_first, uint32_t* q_count, uint32_t* gamma_prime, uint64_t* t, int* launches_scale_down, int* launches_ntt_form) {
    if (!h) return AGX_ERR_NULL_POINTER;
    if (q_first) *q_first = h->view.q_first;
    if (q_count) *q_count = h->view.q_count;
    if (gamma_prime) *gamma_prime = h->gamma_prime;
    if (t) *t = h->view.t;
    if (launches_scale_down) *launches_scale_down = inverse_launches(h->plan) + 1;      // the scaled inverse of the Q slabs, then the streaming kernel
    if (launches_ntt_form) *launches_ntt_form = 1 + forward_launches(h->plan);           // the coefficient-form launch, then the plan's forward on Q
    return AGX_OK;
}

int agx_ntt_plain_scale_up(const agx_ntt_plain* h, const uint64_t* d_m, uint64_t* d_out, uint64_t batch, int out_form, void* stream) {
    return plain_encode_call(h, false, d_m, d_out, batch, out_form, stream);
}

int agx_ntt_plain_lift(const agx_ntt_plain* h, const uint64_t* d_m, uint64_t* d_out, uint64_t batch, int out_form, void* stream) {
    return plain_encode_call(h, true, d_m, d_out, batch, out_form, stream);
}

// The rounding of decryption: the scaled inverse of the Q slabs into the scratch, ONE streaming kernel.
int agx_ntt_plain_scale_down(const agx_ntt_plain* h, const uint64_t* d_x, uint64_t* d_m, uint64_t* d_scratch, uint64_t batch, void* stream) {
    if (int rc = plain_down_rules(h, d_x, d_m, d_scratch, batch)) return rc;
    if (batch == 0) return AGX_OK;
    const agx_ntt_plan* plan = h->plan;
    const plain_view& cv = h->view;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // scratch <- y_i = INTT_i(x_i) gamma t Q_i^-1 mod q_i in [0, q_i): the plan's inverse on Q, its last-stage constants the handle's
    AGX_HIP(run_inverse_on(plan, cv.q_first, cv.q_count, h->d_src_consts, d_x, d_scratch, batch, s));
    AGX_HIP(launch_plain_scale_down(plan->routes.forward, cv, d_scratch, d_m, batch, s));
    return AGX_OK;
}

// BGV decryption, the exact centred conversion Q -> t: the plan's inverse of the Q slabs into the scratch (its own constants: nothing is folded in), ONE
// streaming kernel.  factor's constants are formed here, per call.
int agx_ntt_plain_reduce(const agx_ntt_plain* h, const uint64_t* d_x, uint64_t* d_m, uint64_t* d_scratch, uint64_t factor, uint64_t batch, void* stream) {
    if (int rc = plain_down_rules(h, d_x, d_m, d_scratch, batch)) return rc;
    if (batch == 0) return AGX_OK;
    const agx_ntt_plan* plan = h->plan;
    const plain_view& cv = h->view;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t f = factor % cv.t;
    AGX_HIP(run_inverse_on(plan, cv.q_first, cv.q_count, nullptr, d_x, d_scratch, batch, s));
    AGX_HIP(launch_plain_centred_reduce(plan->routes.forward, cv, d_scratch, d_m, f, shoup_quotient(f, cv.t), batch, s));
    return AGX_OK;
}

// ---- agx_ntt_ckks_*: CKKS encoding and decoding (include/agx_ntt.h has the definition, ckks_arith.hpp the per-word steps) ----

// A CKKS boundary on the current device from its image: the buffers, then the view every call hands to its kernel
static int instantiate_ckks(agx_ntt_ckks** out, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count, const ckks_image& img) {
    std::unique_ptr<agx_ntt_ckks> p(new (std::nothrow) agx_ntt_ckks);
    if (!p) return AGX_ERR_ALLOC;
    p->plan = plan;
    static_assert(sizeof(double2) == 2 * sizeof(double), "the twiddle table is uploaded as double2");
    int rc = p->d_tw.upload(reinterpret_cast<const double2*>(img.tw.data()), img.tw.size() / 2);
    upload_next(rc, p->d_q, img.q);
    if (!img.tri.empty()) upload_next(rc, p->d_tri, img.tri);      // one prime has no Garner constant
    upload_next(rc, p->d_pow2, img.pow2);
    if (rc) return rc;
    ckks_view& v = p->view;
    v.tw = p->d_tw, v.q = p->d_q, v.tri = p->d_tri, v.pow2 = p->d_pow2, v.q_first = q_first, v.q_count = q_count;
    *out = p.release();
    return AGX_OK;
}

// log2 of a legal slot count (a power of two in [1, n / 2]), or -1
static int ckks_log_slots(const agx_ntt_plan* plan, uint32_t slots) {
    if (!is_pow2(slots) || slots > plan->n / 2) return -1;
    return log2u(slots);
}

static bool ckks_scale_ok(double scale) { return scale > 0.0 && scale <= 1.7976931348623157e308; }      // finite and positive; a NaN fails both

// The rules in their order, agx_ntt_plain_create's: NULL; the range; the plan; two equal moduli in the range, a bad modulus.
int agx_ntt_ckks_create(agx_ntt_ckks** h, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count) {
    if (!h) return AGX_ERR_NULL_POINTER;
    *h = nullptr;
    if (!plan) return AGX_ERR_NULL_POINTER;
    if (!primes_in_plan(plan, q_first, q_count) || q_count > AGX_BASIS_MAX_SRC) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    return guarded([&]() -> int {
        ckks_image img;
        if (!prepare_ckks_image(img, &plan->moduli[q_first], q_count, plan->n)) return AGX_ERR_BAD_MODULUS;
        return instantiate_ckks(h, plan, q_first, q_count, img);
    });
}

int agx_ntt_ckks_destroy(agx_ntt_ckks* h) {
    delete h;      // the device memory goes with its owners
    return AGX_OK;
}

int agx_ntt_ckks_info(const agx_ntt_ckks* h, uint32_t* q_first, uint32_t* q_count, uint32_t* max_slots, int* launches_encode_ntt, int* launches_decode_ntt) {
    if (!h) return AGX_ERR_NULL_POINTER;
    if (q_first) *q_first = h->view.q_first;
    if (q_count) *q_count = h->view.q_count;
    if (max_slots) *max_slots = h->plan->n / 2;
    if (launches_encode_ntt) *launches_encode_ntt = 1 + forward_launches(h->plan);      // the coefficient-form launch, then the plan's forward on the range
    if (launches_decode_ntt) *launches_decode_ntt = inverse_launches(h->plan) + 1;      // the plan's inverse on the range, then the decoding kernel
    return AGX_OK;
}

// agx_ntt_plain_scale_up's rules in its order, the handle's arguments (count, slots, scale) first.  Out of place only: d_out's slabs touch d_z nowhere.
int agx_ntt_ckks_encode(const agx_ntt_ckks* h, const double* d_z, uint32_t slots, double scale, uint64_t* d_out, uint64_t batch, uint32_t count, int out_form, void* stream) {
    if (!h || !d_z || !d_out) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = h->plan;
    const ckks_view& cv = h->view;
    if (count == 0 || count > cv.q_count) return AGX_ERR_BAD_ARGUMENT;
    const int log_s = ckks_log_slots(plan, slots);
    if (log_s < 0 || !ckks_scale_ok(scale)) return AGX_ERR_BAD_ARGUMENT;
    if (!form_ok(out_form)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (!aligned8(d_z) || !aligned8(d_out) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    if (!dense_fits(plan->n, count, batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t slab = batch * plan->n;
    if (ranges_touch(addr(d_z), 2 * batch * slots, addr(d_out), count * slab)) return AGX_ERR_BAD_ARGUMENT;      // a pair of doubles is two words
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    AGX_HIP(launch_ckks_encode(plan->log_n, cv, d_z, (uint32_t)log_s, scale, d_out, batch, count, s));
    if (out_form == AGX_FORM_NTT) AGX_HIP(run_forward_on(plan, cv.q_first, count, d_out, d_out, batch, s));      // the call's primes, in place
    return AGX_OK;
}

// agx_ntt_plain_scale_down's rules in its order.  Coefficient form reads d_x itself and never looks at d_scratch.
int agx_ntt_ckks_decode(const agx_ntt_ckks* h, const uint64_t* d_x, int in_form, uint32_t count, double scale, double* d_z, uint32_t slots, uint64_t* d_scratch, uint64_t batch,
                        void* stream) {
    if (!h || !d_x || !d_z || (in_form == AGX_FORM_NTT && !d_scratch)) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = h->plan;
    const ckks_view& cv = h->view;
    if (count == 0 || count > cv.q_count) return AGX_ERR_BAD_ARGUMENT;
    const int log_s = ckks_log_slots(plan, slots);
    if (log_s < 0 || !ckks_scale_ok(scale)) return AGX_ERR_BAD_ARGUMENT;
    if (!form_ok(in_form)) return AGX_ERR_BAD_ARGUMENT;
    const bool ntt = in_form == AGX_FORM_NTT;
    if (int rc = check_plan(plan)) return rc;
    if (!aligned8(d_x) || !aligned8(d_z) || (ntt && !aligned8(d_scratch)) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);      // of x and the scratch ([count][batch][n])
    if (!dense_fits(plan->n, count, batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t words = count * (uint64_t)fl.prime_stride, zwords = 2 * batch * slots;
    // coefficient form has no scratch: x stands in as its own, and the rule is z against x
    if (!scratch_buffers_ok(addr(d_x), words, addr(ntt ? d_scratch : d_x), addr(d_z), zwords)) return AGX_ERR_BAD_ARGUMENT;
    if (ntt && !plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t* coeff = d_x;
    if (ntt) {
        AGX_HIP(run_inverse_on(plan, cv.q_first, count, nullptr, d_x, d_scratch, batch, s));
        coeff = d_scratch;
    }
    AGX_HIP(launch_ckks_decode(plan->log_n, cv, coeff, count, scale, d_z, (uint32_t)log_s, batch, s));
    return AGX_OK;
}

int agx_ntt_ckks_twiddle(uint32_t len, uint32_t j, double out[2]) {
    if (!out) return AGX_ERR_NULL_POINTER;
    return ckks_twiddle(len, j, out) ? AGX_OK : AGX_ERR_BAD_ARGUMENT;
}

// ---- agx_ntt_batch_*: SIMD batching of BFV / BGV (include/agx_ntt.h has the definition, batch_arith.hpp the per-word steps, host_math.hpp the tables) ----

agx_ntt_batch::~agx_ntt_batch() { agx::free_plan(plan); }

// the rules the two calls share behind the NULL rule, agx_ntt_plain_*'s order: the plan's device, alignment and the grid limit, the extent
static int batch_call_rules(const agx_ntt_plan* plan, const void* a, const void* b, const void* c, uint64_t batch) {
    if (int rc = check_plan(plan)) return rc;
    if (!aligned8(a) || !aligned8(b) || !aligned8(c) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    return dense_fits(plan->n, 1, batch) ? AGX_OK : AGX_ERR_BAD_ARGUMENT;
}

// NULL; a size no plan admits, a bad argument; t at or above 2^62, not 1 modulo 2n or composite, a bad modulus; then whatever the plan's creation says
int agx_ntt_batch_create(agx_ntt_batch** h, uint32_t n, uint64_t t) {
    if (!h) return AGX_ERR_NULL_POINTER;
    *h = nullptr;
    if (check_size(n)) return AGX_ERR_BAD_ARGUMENT;
    return guarded([&]() -> int {
        batch_image img;
        switch (prepare_batch_image(img, n, t)) {
            case batch_fault::none: break;
            case batch_fault::root: return AGX_ERR_BAD_ROOT;
            default: return AGX_ERR_BAD_MODULUS;
        }
        std::unique_ptr<agx_ntt_batch> p(new (std::nothrow) agx_ntt_batch);
        if (!p) return AGX_ERR_ALLOC;
        int rc = agx_ntt_plan_create_auto(&p->plan, n, 1, &t, &img.psi);
        upload_next(rc, p->d_slot_to_word, img.slot_to_word), upload_next(rc, p->d_word_to_slot, img.word_to_slot);
        if (rc) return rc;
        p->psi = img.psi;
        p->view = batch_view{p->d_slot_to_word, p->d_word_to_slot, t, img.one_t.p};
        *h = p.release();
        return AGX_OK;
    });
}

int agx_ntt_batch_destroy(agx_ntt_batch* h) {
    delete h;      // the plan and the device memory go with their owner
    return AGX_OK;
}

int agx_ntt_batch_info(const agx_ntt_batch* h, uint32_t* n, uint64_t* t, uint64_t* psi, int* launches_encode, int* launches_decode) {
    if (!h) return AGX_ERR_NULL_POINTER;
    if (n) *n = h->plan->n;
    if (t) *t = h->view.t;
    if (psi) *psi = h->psi;
    if (launches_encode) *launches_encode = 1 + inverse_launches(h->plan);      // the permutation, then the inner plan's inverse in place
    if (launches_decode) *launches_decode = forward_launches(h->plan) + 1;      // the inner plan's forward, then the permutation
    return AGX_OK;
}

int agx_ntt_batch_plan(const agx_ntt_batch* h, agx_ntt_plan** plan) {
    if (!h || !plan) return AGX_ERR_NULL_POINTER;
    *plan = h->plan;
    return AGX_OK;
}

// agx_ntt_plain_scale_up's rules in its order.  Out of place only: d_m touches d_z nowhere.
int agx_ntt_batch_encode(const agx_ntt_batch* h, const uint64_t* d_z, uint64_t* d_m, uint64_t batch, void* stream) {
    if (!h || !d_z || !d_m) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = h->plan;
    if (int rc = batch_call_rules(plan, d_z, d_m, d_m, batch)) return rc;
    const uint64_t words = batch * plan->n;
    if (ranges_touch(addr(d_z), words, addr(d_m), words)) return AGX_ERR_BAD_ARGUMENT;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // m <- the slots modulo t in the forward transform's order, then the inner plan's inverse in place
    AGX_HIP(launch_batch_permute(plan->log_n, h->view, true, d_z, d_m, batch, s));
    AGX_HIP(run_inverse(plan->routes.inverse, d_m, nullptr, d_m, dense(plan, batch), s));
    return AGX_OK;
}

// agx_ntt_plain_scale_down's rules in its order: the scratch IS d_m (the forward then runs in place) or touches none of it; d_z touches neither.
int agx_ntt_batch_decode(const agx_ntt_batch* h, const uint64_t* d_m, uint64_t* d_z, uint64_t* d_scratch, uint64_t batch, void* stream) {
    if (!h || !d_m || !d_z || !d_scratch) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = h->plan;
    if (int rc = batch_call_rules(plan, d_m, d_z, d_scratch, batch)) return rc;
    const uint64_t words = batch * plan->n;
    if (!scratch_buffers_ok(addr(d_m), words, addr(d_scratch), addr(d_z), words)) return AGX_ERR_BAD_ARGUMENT;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    AGX_HIP(run_forward(forward_route(plan, batch), d_m, d_scratch, dense(plan, batch), s));
    AGX_HIP(launch_batch_permute(plan->log_n, h->view, false, d_scratch, d_z, batch, s));
    return AGX_OK;
}

}  // extern "C"
