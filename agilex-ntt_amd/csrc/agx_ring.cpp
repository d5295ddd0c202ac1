// agx_ring.cpp -- the calls that are one streaming kernel over the plan's primes or a range of them: agx_ntt_inner_product and _inner_product_galois,
// agx_ntt_add, _sub, _negate, _add_galois, _tensor and _mul_add_galois, and the samplers agx_ntt_sample_uniform, _ternary and _cbd, which run the plan's
// forward on the range behind their kernel where NTT form is asked for.

#include "plan_internal.hpp"

using namespace agx;

extern "C" {

// agx_ntt_inner_product and agx_ntt_inner_product_galois: one statement of the rules, the Galois element's between the overlap rule and the device's
static int inner_product_call(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_bhat, uint64_t* d_c, uint64_t batch, uint64_t bhat_batch,
                              uint32_t terms, uint32_t outputs, uint32_t galois_elt, void* stream) {
    if (!plan || !d_a || !d_bhat || !d_c) return AGX_ERR_NULL_POINTER;
    if (terms == 0 || terms > AGX_INNER_MAX_TERMS || outputs == 0 || outputs > AGX_INNER_MAX_OUTPUTS || (bhat_batch != batch && bhat_batch != 1)) return AGX_ERR_BAD_ARGUMENT;
    if (!aligned8(d_a) || !aligned8(d_bhat) || !aligned8(d_c)) return AGX_ERR_BAD_ARGUMENT;
    if (!batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;      // from here on batch n < 2^46
    // every operand is one dense range (terms outputs P <= 32 65535 slabs)
    const uint32_t P = plan->num_primes, n = plan->n;
    if (!dense_fits(n, terms * P, batch) || !dense_fits(n, terms * outputs * P, bhat_batch) || !dense_fits(n, outputs * P, batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t slab = batch * n, a_words = terms * P * slab, b_words = (uint64_t)terms * outputs * P * bhat_batch * n, c_words = outputs * P * slab;      // each <= 2^60
    // out of place only, equal pointers included: c_o of a word is written once, but by a thread that other threads' reads of a and bhat do not wait for
    if (ranges_touch(addr(d_c), c_words, addr(d_a), a_words) || ranges_touch(addr(d_c), c_words, addr(d_bhat), b_words)) return AGX_ERR_BAD_ARGUMENT;
    if (!galois_ok(galois_elt, n)) return AGX_ERR_BAD_ARGUMENT;
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

// agx_ntt_add, _sub, _negate, _add_galois and _tensor: one statement of the rules, in the inner products' order.  d_b is d_a for the negation, which has
// one operand; galois_elt is 1 for every call but add_galois.
enum ring_kind { kRingAdd, kRingSub, kRingNegate, kRingAddGalois, kRingTensor };

static int ring_call(ring_kind kind, const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, uint32_t prime_first,
                     uint32_t prime_count, uint32_t galois_elt, void* stream) {
    if (!plan || !d_a || !d_b || !d_c) return AGX_ERR_NULL_POINTER;
    const uint32_t n = plan->n;
    if (!primes_in_plan(plan, prime_first, prime_count)) return AGX_ERR_BAD_ARGUMENT;
    if (!aligned8(d_a) || !aligned8(d_b) || !aligned8(d_c)) return AGX_ERR_BAD_ARGUMENT;
    if (!batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;      // from here on batch n < 2^46
    // every operand is one dense range: prime_count slabs, two and three times as many for the tensor product (at most 3 x 65535)
    const uint32_t in_slabs = (kind == kRingTensor ? 2 : 1) * prime_count, out_slabs = (kind == kRingTensor ? 3 : 1) * prime_count;
    if (!dense_fits(n, in_slabs, batch) || !dense_fits(n, out_slabs, batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t in_words = in_slabs * batch * n, out_words = out_slabs * batch * n;      // each <= 2^60
    // c IS an operand it may equal, or touches nothing of it: add and sub either operand, negate and add_galois a (every work item reads its own words
    // before it writes them).  add_galois reads b across the frame and the tensor product writes three words for two read: c touches those nowhere;
    // g = 1 is agx_ntt_add and takes its rule.
    const bool may_equal_a = kind != kRingTensor, may_equal_b = kind == kRingAdd || kind == kRingSub || kind == kRingNegate || (kind == kRingAddGalois && galois_elt == 1);
    auto apart = [&](const uint64_t* x, bool may_equal) { return (may_equal && x == d_c) || !ranges_touch(addr(d_c), out_words, addr(x), in_words); };
    if (!apart(d_a, may_equal_a) || !apart(d_b, may_equal_b)) return AGX_ERR_BAD_ARGUMENT;
    if (!galois_ok(galois_elt, n)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (batch == 0) return AGX_OK;
    const route& r = plan->routes.forward;      // the whole plan's view: only its constants are read, at [prime_first, prime_first + prime_count)
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (kind == kRingTensor) AGX_HIP(launch_ring_tensor(r, prime_first, prime_count, d_a, d_b, d_c, batch, s));
    else AGX_HIP(launch_ring_linear(r, prime_first, prime_count, kind == kRingSub ? RING_SUB : kind == kRingNegate ? RING_NEG : RING_ADD, d_a, d_b, d_c, batch, galois_elt, s));
    return AGX_OK;
}

int agx_ntt_add(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, uint32_t prime_first, uint32_t prime_count, void* stream) {
    return ring_call(kRingAdd, plan, d_a, d_b, d_c, batch, prime_first, prime_count, 1, stream);
}

int agx_ntt_sub(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, uint32_t prime_first, uint32_t prime_count, void* stream) {
    return ring_call(kRingSub, plan, d_a, d_b, d_c, batch, prime_first, prime_count, 1, stream);
}

int agx_ntt_negate(const agx_ntt_plan* plan, const uint64_t* d_a, uint64_t* d_c, uint64_t batch, uint32_t prime_first, uint32_t prime_count, void* stream) {
    return ring_call(kRingNegate, plan, d_a, d_a, d_c, batch, prime_first, prime_count, 1, stream);
}

int agx_ntt_add_galois(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, uint32_t prime_first, uint32_t prime_count,
                       uint32_t galois_elt, void* stream) {
    return ring_call(kRingAddGalois, plan, d_a, d_b, d_c, batch, prime_first, prime_count, galois_elt, stream);
}

int agx_ntt_tensor(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, uint32_t prime_first, uint32_t prime_count, void* stream) {
    return ring_call(kRingTensor, plan, d_a, d_b, d_c, batch, prime_first, prime_count, 1, stream);
}

// c (+)= w o pi_g(b): the ring calls' rules in their order, the w_batch and accumulate rules beside the range rule.  c touches w nowhere; it touches b
// nowhere either, b being gathered across the frame -- with g = 1 it may be exactly b (every work item reads its own word first).  w and b are only read.
int agx_ntt_mul_add_galois(const agx_ntt_plan* plan, const uint64_t* d_w, uint64_t w_batch, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, uint32_t prime_first,
                           uint32_t prime_count, uint32_t galois_elt, int accumulate, void* stream) {
    if (!plan || !d_w || !d_b || !d_c) return AGX_ERR_NULL_POINTER;
    const uint32_t n = plan->n;
    if (!primes_in_plan(plan, prime_first, prime_count)) return AGX_ERR_BAD_ARGUMENT;
    if ((w_batch != batch && w_batch != 1) || (accumulate != 0 && accumulate != 1)) return AGX_ERR_BAD_ARGUMENT;
    if (!aligned8(d_w) || !aligned8(d_b) || !aligned8(d_c)) return AGX_ERR_BAD_ARGUMENT;
    if (!batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;      // from here on batch n < 2^46
    if (!dense_fits(n, prime_count, batch) || !dense_fits(n, prime_count, w_batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t words = prime_count * batch * n, w_words = prime_count * w_batch * n;      // each <= 2^60
    if (ranges_touch(addr(d_c), words, addr(d_w), w_words)) return AGX_ERR_BAD_ARGUMENT;
    if (!(galois_elt == 1 && d_b == d_c) && ranges_touch(addr(d_c), words, addr(d_b), words)) return AGX_ERR_BAD_ARGUMENT;
    if (!galois_ok(galois_elt, n)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (batch == 0) return AGX_OK;
    AGX_HIP(launch_ring_mul_add_galois(plan->routes.forward, prime_first, prime_count, d_w, w_batch, d_b, d_c, batch, galois_elt, accumulate != 0,
                                       static_cast<hipStream_t>(stream)));
    return AGX_OK;
}

// ---- agx_ntt_sample_*: ChaCha20 uniform, ternary and binomial sampling (include/agx_ntt.h has the definition, sample_arith.hpp the steps) ----

// One statement of the three calls' rules, the ring calls' in their order: NULL; the range; the frame numbers (frame_first + batch <= 2^32, formed without
// overflow); eta; the form; the plan's device; the pointer and the extent.  The key is HOST memory: its 32 bytes become eight little-endian words of the kernel
// arguments, and nothing of it is kept.  NTT form: the coefficient launch, then the plan's forward on the range in place.
static int sample_call(sample_kind kind, const agx_ntt_plan* plan, const uint8_t* key, uint64_t nonce, uint32_t eta, uint64_t* d_out, uint64_t batch, uint64_t frame_first,
                       uint32_t prime_first, uint32_t prime_count, int out_form, void* stream) {
    if (!plan || !key || !d_out) return AGX_ERR_NULL_POINTER;
    const uint32_t n = plan->n;
    if (!primes_in_plan(plan, prime_first, prime_count)) return AGX_ERR_BAD_ARGUMENT;
    constexpr uint64_t kFrames = (uint64_t)1 << 32;
    if (batch > kFrames || frame_first > kFrames - batch) return AGX_ERR_BAD_ARGUMENT;
    if (kind == SAMPLE_CBD && (eta < 1 || eta > 32)) return AGX_ERR_BAD_ARGUMENT;
    if (!form_ok(out_form)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (!aligned8(d_out) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;      // from here on batch n < 2^46
    if (!dense_fits(n, prime_count, batch)) return AGX_ERR_BAD_ARGUMENT;
    if (batch == 0) return AGX_OK;
    uint32_t words[8];
    for (int i = 0; i < 8; ++i) words[i] = (uint32_t)key[4 * i] | (uint32_t)key[4 * i + 1] << 8 | (uint32_t)key[4 * i + 2] << 16 | (uint32_t)key[4 * i + 3] << 24;
    hipStream_t s = static_cast<hipStream_t>(stream);
    AGX_HIP(launch_sample(plan->routes.forward, kind, words, nonce, eta, d_out, batch, frame_first, prime_first, prime_count, s));
    if (out_form == AGX_FORM_NTT) AGX_HIP(run_forward_on(plan, prime_first, prime_count, d_out, d_out, batch, s));
    return AGX_OK;
}

int agx_ntt_sample_uniform(const agx_ntt_plan* plan, const uint8_t key[32], uint64_t nonce, uint64_t* d_out, uint64_t batch, uint64_t frame_first, uint32_t prime_first,
                           uint32_t prime_count, void* stream) {
    return sample_call(SAMPLE_UNIFORM, plan, key, nonce, 0, d_out, batch, frame_first, prime_first, prime_count, AGX_FORM_COEFF, stream);      // no form: uniform words are a uniform ring element in either
}

int agx_ntt_sample_ternary(const agx_ntt_plan* plan, const uint8_t key[32], uint64_t nonce, uint64_t* d_out, uint64_t batch, uint64_t frame_first, uint32_t prime_first,
                           uint32_t prime_count, int out_form, void* stream) {
    return sample_call(SAMPLE_TERNARY, plan, key, nonce, 0, d_out, batch, frame_first, prime_first, prime_count, out_form, stream);
}

int agx_ntt_sample_cbd(const agx_ntt_plan* plan, const uint8_t key[32], uint64_t nonce, uint32_t eta, uint64_t* d_out, uint64_t batch, uint64_t frame_first,
                       uint32_t prime_first, uint32_t prime_count, int out_form, void* stream) {
    return sample_call(SAMPLE_CBD, plan, key, nonce, eta, d_out, batch, frame_first, prime_first, prime_count, out_form, stream);
}

}  // extern "C"
