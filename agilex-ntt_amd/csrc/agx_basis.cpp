// agx_basis.cpp -- agx_ntt_rescale and the calls of a basis (agx_ntt_basis_*): create / create_plain / create_aux / create_quotient, destroy and the info
// calls, extend / extend_exact / extend_mont, mod_down / mod_down_mode and quotient.  Each composes the plan's transforms on a range of its primes
// (run_forward_on / run_inverse_on, plan_internal.hpp) with a coefficient-domain or fused kernel; the key switch (agx_keyswitch.cpp) reaches them
// through the public calls only.
#include <cstdlib>
#include <memory>

#include "host_math.hpp"
#include "plan_internal.hpp"

using namespace agx;

static bool targets_fit_grid(uint32_t T, uint64_t batch, int ppb) { return (uint64_t)T * ((batch + ppb - 1) / ppb) <= 0x7fffffffull; }      // grid limit of the fused kernels: T workgroups per group of ppb frames

// A basis on the current device from its image: the buffers, then the views every call of the basis hands to its kernel
static int instantiate_basis(agx_ntt_basis** out, const agx_ntt_plan* plan, uint32_t src_first, uint32_t dst_first, uint32_t aux_prime, const basis_request& rq,
                             const basis_image& img) {
    std::unique_ptr<agx_ntt_basis> b(new (std::nothrow) agx_ntt_basis);
    if (!b) return AGX_ERR_ALLOC;
    b->plan = plan, b->moddown_legal = img.moddown_legal, b->has_aux = rq.m != 0, b->aux_prime = b->has_aux ? aux_prime : 0;
    int rc = AGX_OK;
    upload_next(rc, b->d_dinv, img.dinv), upload_next(rc, b->d_mat, img.mat), upload_next(rc, b->d_down_mat, img.down_mat), upload_next(rc, b->d_round_src, img.round_src);
    upload_next(rc, b->d_round_dst, img.round_dst), upload_next(rc, b->d_dall, img.dall);
    // the source primes' constants with the inverse's last-stage factors scaled by t^-1 D_i^-1
    upload_next(rc, b->d_src_consts, scaled_consts(plan, src_first, rq.S, img.sn.data(), img.sw.data()));
    if (b->has_aux) {
        upload_next(rc, b->d_aux_row, img.aux_row), upload_next(rc, b->d_aux_corr_exact, img.aux_corr_exact), upload_next(rc, b->d_aux_mdinv, img.aux_mdinv);
        upload_next(rc, b->d_aux_mmat, img.aux_mmat), upload_next(rc, b->d_aux_corr_mont, img.aux_corr_mont);
    }
    if (b->has_aux && rq.quot_t) {
        // the quotient: the target primes' constants and the sources' followed by m's, their last-stage factors the image's
        b->has_quotient = true, b->quot_t = rq.quot_t, b->aux_follows = aux_prime == src_first + rq.S;
        std::vector<prime_consts> qc = scaled_consts(plan, src_first, rq.S, img.quot_sn.data(), img.quot_sw.data());
        qc.push_back(scaled_consts(plan, aux_prime, 1, &img.quot_sn[rq.S], &img.quot_sw[rq.S])[0]);
        upload_next(rc, b->d_quot_mat, img.quot_mat);
        upload_next(rc, b->d_quot_dst_consts, scaled_consts(plan, dst_first, rq.T, img.quot_dn.data(), img.quot_dw.data()));
        upload_next(rc, b->d_quot_src_consts, qc);
    }
    if (rc) return rc;
    basis_view& v = b->view;
    v.dinv = b->d_dinv, v.mat = b->d_mat, v.dall = b->d_dall, v.down_mat = b->d_down_mat, v.round_src = b->d_round_src, v.round_dst = b->d_round_dst;
    v.src_first = src_first, v.src_count = rq.S, v.dst_first = dst_first, v.dst_count = rq.T;
    if (b->has_aux) {
        aux_view& a = b->aux;
        a.row = b->d_aux_row, a.m = rq.m;
        a.exact.dinv = b->d_dinv, a.exact.mat = b->d_mat, a.exact.corr = b->d_aux_corr_exact, a.exact.k = img.k_exact.w, a.exact.kp = img.k_exact.p;
        a.mont.dinv = b->d_aux_mdinv, a.mont.mat = b->d_aux_mmat, a.mont.corr = b->d_aux_corr_mont, a.mont.k = img.k_mont.w, a.mont.kp = img.k_mont.p;
    }
    *out = b.release();
    return AGX_OK;
}

// agx_ntt_basis_create_plain, (t = 1, aux set) agx_ntt_basis_create_aux and (quotient set, quot_t its t: the basis' own t stays 1)
// agx_ntt_basis_create_quotient: validate, build the image, instantiate.  The rules in their order: NULL; the ranges; the plan; sources that share a factor,
// a bad modulus; t = 0, a bad argument; t without an inverse modulo a source, a bad modulus; then the auxiliary prime's: outside the plan or inside a range of
// the basis is a bad argument, a modulus that is a source's or a target's a bad modulus; then the quotient's: more targets than AGX_BASIS_MAX_SRC stands with
// the ranges; ranges that overlap, a bad argument; two equal moduli among the sources, the targets and m, a bad modulus; quot_t = 0, a bad argument.
static int create_basis(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count, uint64_t t,
                        bool aux, uint32_t aux_prime, bool quotient = false, uint64_t quot_t = 0) {
    if (!basis) return AGX_ERR_NULL_POINTER;
    *basis = nullptr;
    if (!plan) return AGX_ERR_NULL_POINTER;
    const uint32_t P = plan->num_primes;
    if (!primes_in_plan(plan, src_first, src_count) || !primes_in_plan(plan, dst_first, dst_count) || src_count > AGX_BASIS_MAX_SRC) return AGX_ERR_BAD_ARGUMENT;
    if (quotient && dst_count > AGX_BASIS_MAX_SRC) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    return guarded([&]() -> int {
        auto inside = [&](uint32_t first, uint32_t count) { return aux_prime >= first && aux_prime - first < count; };
        const bool aux_placed = aux && aux_prime < P && !inside(src_first, src_count) && !inside(dst_first, dst_count);
        std::vector<uint64_t> n_inv, w1n, dst_n_inv, dst_w1n;
        inverse_factors(plan, src_first, src_count, n_inv, w1n);
        basis_request rq{&plan->moduli[src_first], src_count, &plan->moduli[dst_first], dst_count, n_inv.data(), w1n.data(), t, aux_placed ? plan->moduli[aux_prime] : 0};
        if (quotient && aux_placed) {
            inverse_factors(plan, dst_first, dst_count, dst_n_inv, dst_w1n);
            rq.quot_t = quot_t, rq.dst_n_inv = dst_n_inv.data(), rq.dst_w1n = dst_w1n.data();
            rq.aux_n_inv = plan->consts[aux_prime].n_inv, rq.aux_w1n = plan->consts[aux_prime].w1n;
        }
        basis_image img;
        const basis_fault fault = prepare_basis_image(img, rq);      // reports the first of source, t, aux, quotient
        if (fault == basis_fault::source) return AGX_ERR_BAD_MODULUS;
        if (t == 0) return AGX_ERR_BAD_ARGUMENT;
        if (fault == basis_fault::t) return AGX_ERR_BAD_MODULUS;
        if (aux && !aux_placed) return AGX_ERR_BAD_ARGUMENT;
        if (fault == basis_fault::aux) return AGX_ERR_BAD_MODULUS;
        if (quotient) {
            if (src_first < dst_first ? dst_first - src_first < src_count : src_first - dst_first < dst_count) return AGX_ERR_BAD_ARGUMENT;
            // m differs from every source and target (the aux rule above) and the sources from each other (the source rule): targets remain
            for (uint32_t j = 0; j < dst_count; ++j) {
                for (uint32_t k = j + 1; k < dst_count; ++k)
                    if (rq.dst[j] == rq.dst[k]) return AGX_ERR_BAD_MODULUS;
                for (uint32_t i = 0; i < src_count; ++i)
                    if (rq.dst[j] == rq.src[i]) return AGX_ERR_BAD_MODULUS;
            }
            if (fault == basis_fault::quotient) return AGX_ERR_BAD_MODULUS;
            if (quot_t == 0) return AGX_ERR_BAD_ARGUMENT;
        }
        return instantiate_basis(basis, plan, src_first, dst_first, aux_prime, rq, img);
    });
}

extern "C" {

int agx_ntt_rescale(const agx_ntt_plan* plan, const uint64_t* d_x, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, int mode, void* stream) {
    if (!plan || !d_x || !d_out || !d_scratch) return AGX_ERR_NULL_POINTER;
    const uint32_t P = plan->num_primes;
    if (P < 2 || !mode_ok(mode)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);
    int rc = check_plan(plan);
    if (rc || (rc = check_frames(plan, d_x, fl))) return rc;      // x: all P slabs
    if (!aligned8(d_out) || !aligned8(d_scratch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t slab = (uint64_t)fl.prime_stride, head = (P - 1) * slab;
    const uintptr_t x = addr(d_x), x_last = x + 8 * head;      // dense sets, one range each: x is P slabs, out P-1, the scratch one
    if (!down_buffers_ok(x, head, x_last, slab, addr(d_out), addr(d_scratch))) return AGX_ERR_BAD_ARGUMENT;      // ModDown's rule with the last slab as xp
    if (!plan->rescale_legal) return AGX_ERR_BAD_MODULUS;      // some q_i shares a factor with (distinct primes: equals) the last modulus
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    const bool round = mode == AGX_RESCALE_ROUND;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const route& r = plan->routes.rescale; r.rb) {
        // two launches: scratch <- INTT_L(x_L), coefficients in [0, q_L); the lift, the forward transform and (x_i - .) q_L^-1 stay on chip; a wave reads
        // its words of x_i before it writes them
        AGX_HIP(run_inverse_on(plan, P - 1, 1, nullptr, d_x + head, d_scratch, batch, s));
        AGX_HIP(r.rb->launch_rescale(prime_range(r, 0, P - 1), d_x, d_scratch, d_out, fl, round, s));
        return AGX_OK;
    }
    // generic route, no more scratch: out <- INTT(x_0 .. x_{P-2}); scratch <- INTT_L(x_L); out <- (out - lift(scratch)) q_L^-1 in the
    // coefficient domain (a streaming kernel on the view of primes 0 .. P-2); out <- NTT(out)
    AGX_HIP(run_inverse_on(plan, 0, P - 1, nullptr, d_x, d_out, batch, s));
    AGX_HIP(run_inverse_on(plan, P - 1, 1, nullptr, d_x + head, d_scratch, batch, s));
    AGX_HIP(launch_rescale_coeff(prime_range(forward_route(plan, batch), 0, P - 1), d_out, d_scratch, batch, round, s));
    AGX_HIP(run_forward_on(plan, 0, P - 1, d_out, d_out, batch, s));
    return AGX_OK;
}

int agx_ntt_basis_create(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count) {
    return agx_ntt_basis_create_plain(basis, plan, src_first, src_count, dst_first, dst_count, 1);      // t = 1: every constant is what it was without a t
}

int agx_ntt_basis_create_plain(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count,
                               uint64_t t) {
    return create_basis(basis, plan, src_first, src_count, dst_first, dst_count, t, false, 0);
}

int agx_ntt_basis_create_aux(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count,
                             uint32_t aux_prime) {
    return create_basis(basis, plan, src_first, src_count, dst_first, dst_count, 1, true, aux_prime);
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
    return b->view.src_count == 1 || (b->view.src_count == 2 && p->log_n != 12 && p->log_n != 14);
}

int agx_ntt_basis_info(const agx_ntt_basis* basis, uint32_t* src_first, uint32_t* src_count, uint32_t* dst_first, uint32_t* dst_count, int* launches_ntt_form) {
    if (!basis) return AGX_ERR_NULL_POINTER;
    if (src_first) *src_first = basis->view.src_first;
    if (src_count) *src_count = basis->view.src_count;
    if (dst_first) *dst_first = basis->view.dst_first;
    if (dst_count) *dst_count = basis->view.dst_count;
    if (launches_ntt_form) *launches_ntt_form = extend_is_fused(basis) ? 1 : 1 + forward_launches(basis->plan);
    return AGX_OK;
}

// agx_ntt_basis_extend, _extend_exact and _extend_mont behind their own NULL rules (d_xaux null but for exact: an empty range, aligned and touching nothing):
// one statement of the rules, the auxiliary prime's in front of them.  Only the plain conversion has a fused kernel.
enum extend_kind { kExtendPlain, kExtendExact, kExtendMont };

static int extend_call(const agx_ntt_basis* basis, extend_kind kind, const uint64_t* d_x, const uint64_t* d_xaux, uint64_t* d_out, uint64_t batch, int out_form,
                       void* stream) {
    if (kind != kExtendPlain && !basis->has_aux) return AGX_ERR_BAD_ARGUMENT;
    const agx_ntt_plan* plan = basis->plan;
    if (!form_ok(out_form)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    const basis_view& bv = basis->view;
    const uint32_t S = bv.src_count, T = bv.dst_count;
    if (!aligned8(d_x) || !aligned8(d_xaux) || !aligned8(d_out) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);      // of x ([S][batch][n]), xaux ([1][batch][n]) and out ([T][batch][n]) alike
    if (!dense_fits(plan->n, S, batch) || !dense_fits(plan->n, T, batch)) return AGX_ERR_BAD_ARGUMENT;
    // out of place only: every workgroup of a frame reads all S source frames while others already write their targets.  The inputs are only read and
    // may overlap freely.
    const uint64_t slab = batch * plan->n;
    if (ranges_touch(addr(d_x), S * slab, addr(d_out), T * slab) || ranges_touch(addr(d_xaux), kind == kExtendExact ? slab : 0, addr(d_out), T * slab)) return AGX_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const route& r = plan->routes.extend; kind == kExtendPlain && out_form == AGX_FORM_NTT && extend_is_fused(basis)) {
        // one kernel: the conversion and the target prime's forward transform stay on chip
        if (!targets_fit_grid(T, batch, r.rb->ppb)) return AGX_ERR_BAD_ARGUMENT;
        if (batch == 0) return AGX_OK;
        AGX_HIP(r.rb->launch_extend(r, bv, d_x, d_out, fl, s));
        return AGX_OK;
    }
    if (batch == 0) return AGX_OK;
    if (kind == kExtendPlain) AGX_HIP(launch_basis_coeff(plan->routes.forward, bv, d_x, d_out, batch, s));
    else AGX_HIP(launch_basis_aux_coeff(plan->routes.forward, bv, basis->aux, kind == kExtendExact, d_x, d_xaux, d_out, batch, s));
    if (out_form == AGX_FORM_NTT) AGX_HIP(run_forward_on(plan, bv.dst_first, T, d_out, d_out, batch, s));      // the target primes, in place
    return AGX_OK;
}

int agx_ntt_basis_extend(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t batch, int out_form, void* stream) {
    if (!basis || !d_x || !d_out) return AGX_ERR_NULL_POINTER;
    return extend_call(basis, kExtendPlain, d_x, nullptr, d_out, batch, out_form, stream);
}

int agx_ntt_basis_extend_exact(const agx_ntt_basis* basis, const uint64_t* d_x, const uint64_t* d_xaux, uint64_t* d_out, uint64_t batch, int out_form, void* stream) {
    if (!basis || !d_x || !d_xaux || !d_out) return AGX_ERR_NULL_POINTER;
    return extend_call(basis, kExtendExact, d_x, d_xaux, d_out, batch, out_form, stream);
}

int agx_ntt_basis_extend_mont(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t batch, int out_form, void* stream) {
    if (!basis || !d_x || !d_out) return AGX_ERR_NULL_POINTER;
    return extend_call(basis, kExtendMont, d_x, nullptr, d_out, batch, out_form, stream);
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

int agx_ntt_basis_mod_down_info(const agx_ntt_basis* basis, int* launches) {
    if (!basis) return AGX_ERR_NULL_POINTER;
    // fused: the scaled inverse of the source slabs, then moddown_rb2; generic: both inverses, the coefficient-domain step, the forward
    if (launches) *launches = moddown_is_fused(basis) ? inverse_launches(basis->plan) + 1 : 2 * inverse_launches(basis->plan) + 1 + forward_launches(basis->plan);
    return AGX_OK;
}

int agx_ntt_basis_mod_down(const agx_ntt_basis* basis, const uint64_t* d_xq, const uint64_t* d_xp, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream) {
    return agx_ntt_basis_mod_down_mode(basis, d_xq, d_xp, d_out, d_scratch, batch, AGX_RESCALE_FLOOR, stream);
}

// agx_ntt_basis_mod_down's rules in its order, the mode rule right behind the NULL rule (as agx_ntt_rescale has it).  FLOOR launches what mod_down always
// launched; ROUND the kernels with the two per-word steps of moddown_arith.hpp.  The basis' t is in its constants: both modes serve every basis.
int agx_ntt_basis_mod_down_mode(const agx_ntt_basis* basis, const uint64_t* d_xq, const uint64_t* d_xp, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, int mode,
                                void* stream) {
    if (!basis || !d_xq || !d_xp || !d_out || !d_scratch) return AGX_ERR_NULL_POINTER;
    if (!mode_ok(mode)) return AGX_ERR_BAD_ARGUMENT;
    const bool round = mode == AGX_RESCALE_ROUND;
    const agx_ntt_plan* plan = basis->plan;
    if (int rc = check_plan(plan)) return rc;
    const basis_view& bv = basis->view;
    const uint32_t S = bv.src_count, T = bv.dst_count;
    if (!aligned8(d_xq) || !aligned8(d_xp) || !aligned8(d_out) || !aligned8(d_scratch) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);      // of xq and out ([T][batch][n]) and of xp and the scratch ([S][batch][n]) alike
    if (!dense_fits(plan->n, S, batch) || !dense_fits(plan->n, T, batch)) return AGX_ERR_BAD_ARGUMENT;
    const bool fused = moddown_is_fused(basis);
    const route& r = plan->routes.moddown;
    if (fused && !targets_fit_grid(T, batch, r.rb->ppb)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t slab = (uint64_t)fl.prime_stride;      // dense sets, one range each: T slabs for xq and out, S for xp and the scratch
    if (!down_buffers_ok(addr(d_xq), T * slab, addr(d_xp), S * slab, addr(d_out), addr(d_scratch))) return AGX_ERR_BAD_ARGUMENT;
    if (!basis->moddown_legal) return AGX_ERR_BAD_MODULUS;      // some target modulus is a source modulus: D has no inverse there
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // scratch <- y_i = INTT_i(xp_i) t^-1 D_i^-1 mod q_i in [0, q_i): the plan's inverse on the source primes, its last-stage constants the basis'
    if (fused) {
        // two launches: the accumulation, the forward transform and (xq_j - .) D^-1 stay on chip; a wave reads its words of xq_j before it writes them
        AGX_HIP(run_inverse_on(plan, bv.src_first, S, basis->d_src_consts, d_xp, d_scratch, batch, s));
        AGX_HIP(r.rb->launch_moddown(r, bv, d_xq, d_scratch, d_out, fl, round, s));
        return AGX_OK;
    }
    // generic route, no more scratch: out <- INTT(xq) on the target primes; scratch <- the y_i; out <- (out - sum_i y_i D_i) D^-1 in the coefficient
    // domain; out <- NTT(out) in place
    AGX_HIP(run_inverse_on(plan, bv.dst_first, T, nullptr, d_xq, d_out, batch, s));
    AGX_HIP(run_inverse_on(plan, bv.src_first, S, basis->d_src_consts, d_xp, d_scratch, batch, s));
    AGX_HIP(launch_moddown_coeff(plan->routes.forward, bv, d_out, d_scratch, batch, round, s));
    AGX_HIP(run_forward_on(plan, bv.dst_first, T, d_out, d_out, batch, s));
    return AGX_OK;
}

int agx_ntt_basis_aux_info(const agx_ntt_basis* basis, int* has_aux, uint32_t* aux_prime, int* launches_ntt_form) {
    if (!basis) return AGX_ERR_NULL_POINTER;
    if (has_aux) *has_aux = basis->has_aux ? 1 : 0;
    if (aux_prime) *aux_prime = basis->aux_prime;
    if (launches_ntt_form) *launches_ntt_form = 1 + forward_launches(basis->plan);      // the coefficient-form launch, then the plan's forward on the targets
    return AGX_OK;
}

// The basis of agx_ntt_basis_create_aux(plan, b_first, b_count, q_first, q_count, aux_prime) -- sources B, targets Q, t = 1 in every call it had -- with the
// constants of agx_ntt_basis_quotient for this t.
int agx_ntt_basis_create_quotient(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t b_first, uint32_t b_count, uint32_t q_first, uint32_t q_count,
                                  uint32_t aux_prime, uint64_t t) {
    return create_basis(basis, plan, b_first, b_count, q_first, q_count, 1, true, aux_prime, true, t);
}

// the inverse launches of one quotient call: Q, then Bsk -- in one where m is the plan prime right behind B, else B and m apart
static int quotient_inverses(const agx_ntt_basis* b) { return b->aux_follows ? 2 : 3; }

int agx_ntt_basis_quotient_info(const agx_ntt_basis* basis, int* has_quotient, uint64_t* t, int* launches) {
    if (!basis) return AGX_ERR_NULL_POINTER;
    if (has_quotient) *has_quotient = basis->has_quotient ? 1 : 0;
    if (t) *t = basis->quot_t;
    if (launches) *launches = quotient_inverses(basis) * inverse_launches(basis->plan) + 1 + forward_launches(basis->plan);
    return AGX_OK;
}

// Steps 4 to 7 of a BFV multiplication in the coefficient domain (include/agx_ntt.h has the contract): the scaled inverses of the Q slabs and of the Bsk
// slabs into the scratch, ONE kernel for the fast floor and the Shenoy-Kumaresan return, the plan's forward on Q in place in d_out.
int agx_ntt_basis_quotient(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream) {
    if (!basis || !d_x || !d_out || !d_scratch) return AGX_ERR_NULL_POINTER;
    if (!basis->has_quotient) return AGX_ERR_BAD_ARGUMENT;
    const agx_ntt_plan* plan = basis->plan;
    if (int rc = check_plan(plan)) return rc;
    const basis_view& bv = basis->view;
    const uint32_t K = bv.src_count, L = bv.dst_count, W = L + K + 1;
    if (!aligned8(d_x) || !aligned8(d_out) || !aligned8(d_scratch) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);      // of x and the scratch ([W][batch][n]) and of out ([L][batch][n]) alike
    if (!dense_fits(plan->n, W, batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t slab = (uint64_t)fl.prime_stride;
    if (!scratch_buffers_ok(addr(d_x), W * slab, addr(d_scratch), addr(d_out), L * slab)) return AGX_ERR_BAD_ARGUMENT;      // every inverse may run in place
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // scratch <- the y_i on Q, then the s_j on B and s_m: the plan's inverse on those views, its last-stage constants the basis'
    auto scaled_inverse = [&](uint32_t first, uint32_t count, const prime_consts* consts, uint64_t at) {
        return run_inverse_on(plan, first, count, consts, d_x + at * slab, d_scratch + at * slab, batch, s);
    };
    AGX_HIP(scaled_inverse(bv.dst_first, L, basis->d_quot_dst_consts, 0));
    AGX_HIP(scaled_inverse(bv.src_first, basis->aux_follows ? K + 1 : K, basis->d_quot_src_consts, L));
    if (!basis->aux_follows) AGX_HIP(scaled_inverse(basis->aux_prime, 1, basis->d_quot_src_consts + K, L + K));
    AGX_HIP(launch_basis_quotient(plan->routes.forward, bv, basis->aux, basis->d_quot_mat, d_scratch, d_out, batch, s));
    AGX_HIP(run_forward_on(plan, bv.dst_first, L, d_out, d_out, batch, s));
    return AGX_OK;
}

}  // extern "C"
