// agx_keyswitch.cpp -- the hybrid key switch (agx_ntt_keyswitch_*): create / create_plain, destroy, the info and size calls, apply, and its halves
// decompose, apply_decomposed, accumulate_decomposed and mod_down.  A host composition of the plan's inverse, the inner-product kernels and the public
// calls of its bases (agx_ntt_basis_create*, _extend, _mod_down and their info calls, agx_basis.cpp).
#include <memory>

#include "host_math.hpp"
#include "plan_internal.hpp"

using namespace agx;

extern "C" {

int agx_ntt_keyswitch_create(agx_ntt_keyswitch** ks, const agx_ntt_plan* plan, uint32_t q_count, uint32_t p_first, uint32_t p_count, uint32_t alpha) {
    return agx_ntt_keyswitch_create_plain(ks, plan, q_count, p_first, p_count, alpha, 1);
}

// agx_ntt_keyswitch_create with the ModDown basis made by agx_ntt_basis_create_plain(..., t); the ModUp bases are the ordinary ones.  t = 0 is a bad
// argument behind keyswitch_create's own rules; a t without an inverse modulo a special prime is what the ModDown basis reports: a bad modulus.
int agx_ntt_keyswitch_create_plain(agx_ntt_keyswitch** ks, const agx_ntt_plan* plan, uint32_t q_count, uint32_t p_first, uint32_t p_count, uint32_t alpha, uint64_t t) {
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
    if (t == 0) return AGX_ERR_BAD_ARGUMENT;
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
        if (int rc = agx_ntt_basis_create_plain(&k->down, plan, p_first, p_count, 0, q_count, t)) return rc;
        *ks = k.release();
        return AGX_OK;
    });
}

int agx_ntt_keyswitch_destroy(agx_ntt_keyswitch* ks) {
    delete ks;      // the bases go with it
    return AGX_OK;
}

// kernel launches of the two halves of an apply call, each under the plan's current variant: the inverse on Q + what every ModUp basis reports; the
// inner product + two ModDown calls
static int decompose_launches(const agx_ntt_keyswitch* ks) {
    int extend[2 * kKeyswitchMaxDigits];
    for (size_t i = 0; i < ks->up.size(); ++i) (void)agx_ntt_basis_info(ks->up[i], nullptr, nullptr, nullptr, nullptr, &extend[i]);
    return keyswitch_launches_decompose(inverse_launches(ks->plan), extend, (uint32_t)ks->up.size());
}
static int apply_decomposed_launches(const agx_ntt_keyswitch* ks) {
    int down = 0;
    (void)agx_ntt_basis_mod_down_info(ks->down, &down);
    return keyswitch_launches_apply_decomposed(down);
}

int agx_ntt_keyswitch_info(const agx_ntt_keyswitch* ks, uint32_t* q_count, uint32_t* p_first, uint32_t* p_count, uint32_t* alpha, uint32_t* digits, int* launches) {
    if (!ks) return AGX_ERR_NULL_POINTER;
    if (q_count) *q_count = ks->shape.q_count;
    if (p_first) *p_first = ks->shape.p_first;
    if (p_count) *p_count = ks->shape.p_count;
    if (alpha) *alpha = ks->shape.alpha;
    if (digits) *digits = ks->shape.digits();
    if (launches) *launches = decompose_launches(ks) + apply_decomposed_launches(ks);      // what agx_ntt_keyswitch_hoisted_info reports, summed
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
    if (launches_decompose) *launches_decompose = decompose_launches(ks);
    if (launches_apply_decomposed) *launches_apply_decomposed = apply_decomposed_launches(ks);
    return AGX_OK;
}

// Steps 1 and 2 of a key switch, every argument checked by the caller: coeff [Q][batch][n] <- INTT(chat), ext [digits][A][batch][n] <- ModUp of every digit
static int keyswitch_decompose_steps(const agx_ntt_keyswitch* ks, const uint64_t* d_chat, uint64_t* ext, uint64_t* coeff, uint64_t batch, void* stream) {
    const agx_ntt_plan* plan = ks->plan;
    const keyswitch_shape& k = ks->shape;
    const uint32_t Q = k.q_count, A = k.active(), digits = k.digits();
    const uint64_t slab = batch * plan->n;
    // (1) coeff_j <- INTT_j(chat_j) in [0, q_j): the plan's inverse on the view of primes [0, Q), as ModDown runs it on its sources: no second plan
    AGX_HIP(run_inverse_on(plan, 0, Q, nullptr, d_chat, coeff, batch, static_cast<hipStream_t>(stream)));
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

// Step 3, every argument checked by the caller: acc_o [A][batch][n] <- (accumulate ? acc_o : 0) + weight o sum_d pi_g(ext_d) o key_{d,o} over the active
// primes: one launch, the key broadcast over the batch; g = 1 is the un-gathered kernel.  Without a weight and an old acc it is the inner product itself,
// and launches that kernel: what apply and apply_decomposed run is what they ran before this step had a weight.
static int keyswitch_accumulate_step(const agx_ntt_keyswitch* ks, const uint64_t* ext, const uint64_t* d_keyhat, const uint64_t* weight, uint64_t weight_batch,
                                     uint64_t* acc, uint64_t batch, uint32_t galois_elt, bool accumulate, void* stream) {
    const agx_ntt_plan* plan = ks->plan;
    const keyswitch_shape& k = ks->shape;
    const inner_primes active{k.active(), k.q_count, k.p_first - k.q_count};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!weight && !accumulate) AGX_HIP(launch_inner_product_galois(plan->routes.forward, active, ext, d_keyhat, acc, batch, 1, k.digits(), 2, galois_elt, s));
    else AGX_HIP(launch_inner_weighted(plan->routes.forward, active, ext, d_keyhat, weight, weight_batch, acc, batch, k.digits(), galois_elt, accumulate, s));
    return AGX_OK;
}

// Step 4, every argument checked by the caller: out_o [Q][batch][n] <- ModDown of acc_o, its special slabs given up as the scratch
static int keyswitch_mod_down_step(const agx_ntt_keyswitch* ks, uint64_t* acc, uint64_t* d_out, uint64_t batch, void* stream) {
    const uint32_t Q = ks->shape.q_count, A = ks->shape.active();
    const uint64_t slab = batch * ks->plan->n;
    for (uint32_t o = 0; o < 2; ++o) {
        uint64_t* xq = acc + (uint64_t)o * A * slab;
        if (int rc = agx_ntt_basis_mod_down(ks->down, xq, xq + Q * slab, d_out + o * Q * slab, xq + Q * slab, batch, stream)) return rc;
    }
    return AGX_OK;
}

// Steps 3 and 4: the two halves with no weight and nothing accumulated
static int keyswitch_apply_steps(const agx_ntt_keyswitch* ks, const uint64_t* ext, const uint64_t* d_keyhat, uint64_t* d_out, uint64_t* acc, uint64_t batch,
                                 uint32_t galois_elt, void* stream) {
    if (int rc = keyswitch_accumulate_step(ks, ext, d_keyhat, nullptr, 0, acc, batch, galois_elt, false, stream)) return rc;
    return keyswitch_mod_down_step(ks, acc, d_out, batch, stream);
}

// the rules the key-switch calls share, after the NULL rule and the 2^60 limits: alignment, the two grid limits, and no two of the call's `count` buffers touching
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
    if (!galois_ok(galois_elt, plan->n)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;      // ModDown runs the plan's inverse
    if (batch == 0) return AGX_OK;
    return keyswitch_apply_steps(ks, d_ext, d_keyhat, d_out, d_scratch, batch, galois_elt, stream);
}

// Step 3 alone, weighted and accumulating: apply_decomposed's rules in its order, the weight one more buffer of the overlap rule, the weight_batch and
// accumulate rules in front of it.  It runs no inverse: a forward-only plan serves.
int agx_ntt_keyswitch_accumulate_decomposed(const agx_ntt_keyswitch* ks, const uint64_t* d_ext, const uint64_t* d_keyhat, const uint64_t* d_weight, uint64_t weight_batch,
                                            uint64_t* d_acc, uint64_t batch, uint32_t galois_elt, int accumulate, void* stream) {
    if (!ks || !d_ext || !d_keyhat || !d_acc) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = ks->plan;
    const keyswitch_shape& k = ks->shape;
    keyswitch_hoisted part;
    if (!keyswitch_hoisted_partition(k, plan->n, batch, &part)) return AGX_ERR_BAD_ARGUMENT;
    if ((d_weight && weight_batch != batch && weight_batch != 1) || (accumulate != 0 && accumulate != 1)) return AGX_ERR_BAD_ARGUMENT;
    // the weight's extent is half of acc's or smaller; without a weight it is an empty range, which touches nothing and is aligned
    const uintptr_t base[4] = {addr(d_ext), addr(d_keyhat), addr(d_acc), addr(d_weight)};
    const uint64_t words[4] = {part.ext, (uint64_t)k.digits() * 2 * k.active() * plan->n, part.apply_scratch, d_weight ? k.active() * weight_batch * plan->n : 0};
    if (!keyswitch_buffers_ok(ks, batch, base, words, 4)) return AGX_ERR_BAD_ARGUMENT;
    if (!galois_ok(galois_elt, plan->n)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (batch == 0) return AGX_OK;
    return keyswitch_accumulate_step(ks, d_ext, d_keyhat, d_weight, weight_batch, d_acc, batch, galois_elt, accumulate != 0, stream);
}

// Step 4 alone: apply_decomposed's rules without the key and the Galois element
int agx_ntt_keyswitch_mod_down(const agx_ntt_keyswitch* ks, uint64_t* d_acc, uint64_t* d_out, uint64_t batch, void* stream) {
    if (!ks || !d_acc || !d_out) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = ks->plan;
    keyswitch_hoisted part;
    if (!keyswitch_hoisted_partition(ks->shape, plan->n, batch, &part)) return AGX_ERR_BAD_ARGUMENT;
    const uintptr_t base[2] = {addr(d_acc), addr(d_out)};
    const uint64_t words[2] = {part.apply_scratch, 2 * part.decompose_scratch};
    if (!keyswitch_buffers_ok(ks, batch, base, words, 2)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;      // ModDown runs the plan's inverse
    if (batch == 0) return AGX_OK;
    return keyswitch_mod_down_step(ks, d_acc, d_out, batch, stream);
}

int agx_ntt_keyswitch_apply(const agx_ntt_keyswitch* ks, const uint64_t* d_chat, const uint64_t* d_keyhat, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream) {
    if (!ks || !d_chat || !d_keyhat || !d_out || !d_scratch) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = ks->plan;
    const keyswitch_shape& k = ks->shape;
    keyswitch_scratch part;
    if (!keyswitch_scratch_partition(k, plan->n, batch, &part)) return AGX_ERR_BAD_ARGUMENT;      // every extent below is a part of the scratch's or smaller
    const uint64_t chat_words = k.q_count * batch * plan->n;      // [Q][batch][n], the size of the coeff part
    const uintptr_t base[4] = {addr(d_chat), addr(d_keyhat), addr(d_out), addr(d_scratch)};
    const uint64_t words[4] = {chat_words, (uint64_t)k.digits() * 2 * k.active() * plan->n, 2 * chat_words, part.total};
    if (!keyswitch_buffers_ok(ks, batch, base, words, 4)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    // the two halves on the three parts of the one scratch, with g = 1: the un-gathered inner product
    if (int rc = keyswitch_decompose_steps(ks, d_chat, d_scratch + part.ext, d_scratch + part.coeff, batch, stream)) return rc;
    return keyswitch_apply_steps(ks, d_scratch + part.ext, d_keyhat, d_out, d_scratch + part.acc, batch, 1, stream);
}

}  // extern "C"
