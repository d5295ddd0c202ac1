// agx_rns.cpp -- the RNS calls of include/agx_ntt.h: rescale, basis extension and ModDown, the inner products, the ring arithmetic on a range of the
// plan's primes (add, sub, negate, add_galois, tensor, mul_add_galois: one streaming kernel each) and the key switch, whole, in two halves, and with its
// second half in two (accumulate_decomposed: the weighted, accumulating inner product; keyswitch_mod_down), and BFV's plaintext boundary (agx_ntt_plain_*:
// scale_up, lift, scale_down, and reduce: BGV decryption), the samplers (agx_ntt_sample_*: one streaming kernel each), CKKS encoding and, at the end of the
// file, batching (agx_ntt_batch_*: a handle that owns its own one-prime plan).  Each of the others composes the
// plan's transforms (run_forward / run_inverse on views of its routes, plan_internal.hpp) with a coefficient-domain or fused kernel; plans, routes and
// the transform calls themselves live in agx_ntt.cpp.
#include <cstdlib>
#include <memory>

#include "host_math.hpp"
#include "plan_internal.hpp"

using namespace agx;

static bool targets_fit_grid(uint32_t T, uint64_t batch, int ppb) { return (uint64_t)T * ((batch + ppb - 1) / ppb) <= 0x7fffffffull; }      // grid limit of the fused kernels: T workgroups per group of ppb frames
static bool dense_fits(uint32_t n, uint32_t slabs, uint64_t frames) { return layout_fits(n, slabs, frames, (int64_t)(frames * n), (int64_t)n); }      // one dense range of slabs x frames x n words (formed in 128 bits)

// A basis on the current device from its image: the buffers, then the views every call of the basis hands to its kernel
static int instantiate_basis(agx_ntt_basis** out, const agx_ntt_plan* plan, uint32_t src_first, uint32_t dst_first, uint32_t aux_prime, const basis_request& rq,
                             const basis_image& img) {
    std::unique_ptr<agx_ntt_basis> b(new (std::nothrow) agx_ntt_basis);
    if (!b) return AGX_ERR_ALLOC;
    b->plan = plan, b->moddown_legal = img.moddown_legal, b->has_aux = rq.m != 0, b->aux_prime = b->has_aux ? aux_prime : 0;
    // the source primes' constants (the plan's host copy) with the inverse's last-stage factors scaled by t^-1 D_i^-1
    std::vector<prime_consts> sc(plan->consts.begin() + src_first, plan->consts.begin() + src_first + rq.S);
    for (uint32_t i = 0; i < rq.S; ++i) sc[i].n_inv = img.sn[i].w, sc[i].n_inv_p = img.sn[i].p, sc[i].w1n = img.sw[i].w, sc[i].w1n_p = img.sw[i].p;
    int rc = AGX_OK;
    auto put = [&](device_buf<ulonglong2>& to, const std::vector<shoup_pair>& pairs) { if (rc == AGX_OK) rc = upload_pairs(to, pairs); };
    put(b->d_dinv, img.dinv), put(b->d_mat, img.mat), put(b->d_down_mat, img.down_mat), put(b->d_round_src, img.round_src);
    if (rc == AGX_OK) rc = b->d_round_dst.upload(img.round_dst);
    put(b->d_dall, img.dall);
    if (rc == AGX_OK) rc = b->d_src_consts.upload(sc);
    if (b->has_aux) put(b->d_aux_row, img.aux_row), put(b->d_aux_corr_exact, img.aux_corr_exact), put(b->d_aux_mdinv, img.aux_mdinv), put(b->d_aux_mmat, img.aux_mmat), put(b->d_aux_corr_mont, img.aux_corr_mont);
    if (b->has_aux && rq.quot_t) {
        // the quotient: the target primes' constants and the sources' followed by m's, their last-stage factors the image's
        b->has_quotient = true, b->quot_t = rq.quot_t, b->aux_follows = aux_prime == src_first + rq.S;
        std::vector<prime_consts> dc(plan->consts.begin() + dst_first, plan->consts.begin() + dst_first + rq.T), qc(sc);
        qc.push_back(plan->consts[aux_prime]);
        auto scale = [](prime_consts& c, const shoup_pair& n, const shoup_pair& w) { c.n_inv = n.w, c.n_inv_p = n.p, c.w1n = w.w, c.w1n_p = w.p; };
        for (uint32_t j = 0; j < rq.T; ++j) scale(dc[j], img.quot_dn[j], img.quot_dw[j]);
        for (uint32_t i = 0; i <= rq.S; ++i) scale(qc[i], img.quot_sn[i], img.quot_sw[i]);
        put(b->d_quot_mat, img.quot_mat);
        if (rc == AGX_OK) rc = b->d_quot_dst_consts.upload(dc);
        if (rc == AGX_OK) rc = b->d_quot_src_consts.upload(qc);
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
    auto in_plan = [&](uint32_t first, uint32_t count) { return count >= 1 && count <= P && first <= P - count; };
    if (!in_plan(src_first, src_count) || !in_plan(dst_first, dst_count) || src_count > AGX_BASIS_MAX_SRC) return AGX_ERR_BAD_ARGUMENT;
    if (quotient && dst_count > AGX_BASIS_MAX_SRC) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    return guarded([&]() -> int {
        auto inside = [&](uint32_t first, uint32_t count) { return aux_prime >= first && aux_prime - first < count; };
        const bool aux_placed = aux && aux_prime < P && !inside(src_first, src_count) && !inside(dst_first, dst_count);
        std::vector<uint64_t> n_inv(src_count), w1n(src_count);
        for (uint32_t i = 0; i < src_count; ++i) n_inv[i] = plan->consts[src_first + i].n_inv, w1n[i] = plan->consts[src_first + i].w1n;
        basis_request rq{&plan->moduli[src_first], src_count, &plan->moduli[dst_first], dst_count, n_inv.data(), w1n.data(), t, aux_placed ? plan->moduli[aux_prime] : 0};
        std::vector<uint64_t> dst_n_inv(dst_count), dst_w1n(dst_count);
        if (quotient && aux_placed) {
            for (uint32_t j = 0; j < dst_count; ++j) dst_n_inv[j] = plan->consts[dst_first + j].n_inv, dst_w1n[j] = plan->consts[dst_first + j].w1n;
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
    if (P < 2 || (mode != AGX_RESCALE_FLOOR && mode != AGX_RESCALE_ROUND)) return AGX_ERR_BAD_ARGUMENT;
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
    // scratch <- INTT_L(x_L), coefficients in [0, q_L): the plan's inverse on the view of prime P-1
    const route last = prime_range(plan->routes.inverse, P - 1, P);
    if (const route& r = plan->routes.rescale; r.rb) {
        // two launches: the lift, the forward transform and (x_i - .) q_L^-1 stay on chip; a wave reads its words of x_i before it writes them
        AGX_HIP(run_inverse(last, d_x + head, nullptr, d_scratch, fl, s));
        AGX_HIP(r.rb->launch_rescale(prime_range(r, 0, P - 1), d_x, d_scratch, d_out, fl, round, s));
        return AGX_OK;
    }
    // generic route, no more scratch: out <- INTT(x_0 .. x_{P-2}); scratch <- INTT_L(x_L); out <- (out - lift(scratch)) q_L^-1 in the
    // coefficient domain; out <- NTT(out)
    AGX_HIP(run_inverse(prime_range(plan->routes.inverse, 0, P - 1), d_x, nullptr, d_out, fl, s));
    AGX_HIP(run_inverse(last, d_x + head, nullptr, d_scratch, fl, s));
    const route head_route = prime_range(forward_route(plan, batch), 0, P - 1);
    AGX_HIP(launch_rescale_coeff(head_route, d_out, d_scratch, batch, round, s));
    AGX_HIP(run_forward(head_route, d_out, d_out, fl, s));
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
    if (out_form != AGX_FORM_COEFF && out_form != AGX_FORM_NTT) return AGX_ERR_BAD_ARGUMENT;
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
    // the plan's forward on the view of the target primes, in place
    if (out_form == AGX_FORM_NTT) AGX_HIP(run_forward(prime_range(forward_route(plan, batch), bv.dst_first, bv.dst_first + T), d_out, d_out, fl, s));
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
    if (mode != AGX_RESCALE_FLOOR && mode != AGX_RESCALE_ROUND) return AGX_ERR_BAD_ARGUMENT;
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
    // scratch <- y_i = INTT_i(xp_i) t^-1 D_i^-1 mod q_i in [0, q_i): the plan's inverse on the view of the source primes, its last-stage constants the basis'
    route scaled = prime_range(plan->routes.inverse, bv.src_first, bv.src_first + S);
    scaled.consts = basis->d_src_consts;
    if (fused) {
        // two launches: the accumulation, the forward transform and (xq_j - .) D^-1 stay on chip; a wave reads its words of xq_j before it writes them
        AGX_HIP(run_inverse(scaled, d_xp, nullptr, d_scratch, fl, s));
        AGX_HIP(r.rb->launch_moddown(r, bv, d_xq, d_scratch, d_out, fl, round, s));
        return AGX_OK;
    }
    // generic route, no more scratch: out <- INTT(xq) on the target primes; scratch <- the y_i; out <- (out - sum_i y_i D_i) D^-1 in the coefficient
    // domain; out <- NTT(out) in place
    AGX_HIP(run_inverse(prime_range(plan->routes.inverse, bv.dst_first, bv.dst_first + T), d_xq, nullptr, d_out, fl, s));
    AGX_HIP(run_inverse(scaled, d_xp, nullptr, d_scratch, fl, s));
    AGX_HIP(launch_moddown_coeff(plan->routes.forward, bv, d_out, d_scratch, batch, round, s));
    AGX_HIP(run_forward(prime_range(forward_route(plan, batch), bv.dst_first, bv.dst_first + T), d_out, d_out, fl, s));
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
    // the scratch IS x (every inverse then runs in place, as agx_ntt_inverse may) or touches none of it; out touches neither
    const uint64_t slab = (uint64_t)fl.prime_stride;
    if (d_scratch != d_x && ranges_touch(addr(d_scratch), W * slab, addr(d_x), W * slab)) return AGX_ERR_BAD_ARGUMENT;
    if (ranges_touch(addr(d_out), L * slab, addr(d_x), W * slab) || ranges_touch(addr(d_out), L * slab, addr(d_scratch), W * slab)) return AGX_ERR_BAD_ARGUMENT;
    if (!plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // scratch <- the y_i on Q, then the s_j on B and s_m: the plan's inverse on those views, its last-stage constants the basis'
    auto scaled_inverse = [&](uint32_t first, uint32_t count, const prime_consts* consts, uint64_t at) {
        route r = prime_range(plan->routes.inverse, first, first + count);
        r.consts = consts;
        return run_inverse(r, d_x + at * slab, nullptr, d_scratch + at * slab, fl, s);
    };
    AGX_HIP(scaled_inverse(bv.dst_first, L, basis->d_quot_dst_consts, 0));
    AGX_HIP(scaled_inverse(bv.src_first, basis->aux_follows ? K + 1 : K, basis->d_quot_src_consts, L));
    if (!basis->aux_follows) AGX_HIP(scaled_inverse(basis->aux_prime, 1, basis->d_quot_src_consts + K, L + K));
    AGX_HIP(launch_basis_quotient(plan->routes.forward, bv, basis->aux, basis->d_quot_mat, d_scratch, d_out, batch, s));
    AGX_HIP(run_forward(prime_range(forward_route(plan, batch), bv.dst_first, bv.dst_first + L), d_out, d_out, fl, s));
    return AGX_OK;
}

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

}  // extern "C"

// agx_ntt_add, _sub, _negate, _add_galois and _tensor: one statement of the rules, in the inner products' order.  d_b is d_a for the negation, which has
// one operand; galois_elt is 1 for every call but add_galois.
enum ring_kind { kRingAdd, kRingSub, kRingNegate, kRingAddGalois, kRingTensor };

static int ring_call(ring_kind kind, const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, uint32_t prime_first,
                     uint32_t prime_count, uint32_t galois_elt, void* stream) {
    if (!plan || !d_a || !d_b || !d_c) return AGX_ERR_NULL_POINTER;
    const uint32_t P = plan->num_primes, n = plan->n;
    if (prime_count == 0 || prime_count > P || prime_first > P - prime_count) return AGX_ERR_BAD_ARGUMENT;
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

extern "C" {

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
    const uint32_t P = plan->num_primes, n = plan->n;
    if (prime_count == 0 || prime_count > P || prime_first > P - prime_count) return AGX_ERR_BAD_ARGUMENT;
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
    AGX_HIP(run_inverse(prime_range(plan->routes.inverse, 0, Q), d_chat, nullptr, coeff, dense(plan, batch), static_cast<hipStream_t>(stream)));
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

// ---- agx_ntt_plain_*: BFV's plaintext boundary (include/agx_ntt.h has the contract, plain_arith.hpp the formulas) ----

// A plaintext boundary on the current device from its image: the buffers, then the view every call hands to its kernel
static int instantiate_plain(agx_ntt_plain** out, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count, uint32_t gamma_prime, uint64_t t, const plain_image& img) {
    std::unique_ptr<agx_ntt_plain> p(new (std::nothrow) agx_ntt_plain);
    if (!p) return AGX_ERR_ALLOC;
    p->plan = plan, p->gamma_prime = gamma_prime;
    std::vector<prime_consts> sc(plan->consts.begin() + q_first, plan->consts.begin() + q_first + q_count);
    for (uint32_t i = 0; i < q_count; ++i) sc[i].n_inv = img.sn[i].w, sc[i].n_inv_p = img.sn[i].p, sc[i].w1n = img.sw[i].w, sc[i].w1n_p = img.sw[i].p;
    int rc = AGX_OK;
    auto put = [&](device_buf<ulonglong2>& to, const std::vector<shoup_pair>& pairs) { if (rc == AGX_OK) rc = upload_pairs(to, pairs); };
    put(p->d_up, img.up), put(p->d_one, img.one), put(p->d_row_t, img.row_t), put(p->d_row_g, img.row_g);
    put(p->d_radix_t, img.radix_t);
    if (!img.tri.empty()) put(p->d_tri, img.tri);      // one prime has no Garner constant
    if (rc == AGX_OK) rc = p->d_q.upload(img.q);
    if (rc == AGX_OK) rc = p->d_src_consts.upload(sc);
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
    // the scratch IS x (the inverse then runs in place, as agx_ntt_inverse may) or touches none of it; m touches neither
    const uint64_t slab = (uint64_t)fl.prime_stride;
    if (d_scratch != d_x && ranges_touch(addr(d_scratch), L * slab, addr(d_x), L * slab)) return AGX_ERR_BAD_ARGUMENT;
    if (ranges_touch(addr(d_m), slab, addr(d_x), L * slab) || ranges_touch(addr(d_m), slab, addr(d_scratch), L * slab)) return AGX_ERR_BAD_ARGUMENT;
    return plan->has_inverse ? AGX_OK : AGX_ERR_NO_INVERSE;
}

// agx_ntt_plain_scale_up and _lift: one statement of the rules, in extend_call's order.  Out of place only: d_out's L slabs touch d_m nowhere.
static int plain_encode_call(const agx_ntt_plain* h, bool lift, const uint64_t* d_m, uint64_t* d_out, uint64_t batch, int out_form, void* stream) {
    if (!h || !d_m || !d_out) return AGX_ERR_NULL_POINTER;
    const agx_ntt_plan* plan = h->plan;
    if (out_form != AGX_FORM_COEFF && out_form != AGX_FORM_NTT) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    const plain_view& cv = h->view;
    const uint32_t L = cv.q_count;
    if (!aligned8(d_m) || !aligned8(d_out) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);      // of m ([1][batch][n]) and out ([L][batch][n]) alike
    if (!dense_fits(plan->n, L, batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t slab = batch * plan->n;
    if (ranges_touch(addr(d_m), slab, addr(d_out), L * slab)) return AGX_ERR_BAD_ARGUMENT;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    AGX_HIP(launch_plain_encode(plan->routes.forward, cv, lift, d_m, d_out, batch, s));
    // the plan's forward on the view of Q, in place
    if (out_form == AGX_FORM_NTT) AGX_HIP(run_forward(prime_range(forward_route(plan, batch), cv.q_first, cv.q_first + L), d_out, d_out, fl, s));
    return AGX_OK;
}

extern "C" {

// The rules in their order, agx_ntt_basis_create_aux's: NULL; the range and gamma's place, a bad argument; the plan; two moduli of Q that share a factor, gamma
// sharing one with a modulus of Q, a bad modulus; t outside [2, 2^62), a bad argument; t sharing a factor with some q_i, then with gamma, a bad modulus.
int agx_ntt_plain_create(agx_ntt_plain** h, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count, uint32_t gamma_prime, uint64_t t) {
    if (!h) return AGX_ERR_NULL_POINTER;
    *h = nullptr;
    if (!plan) return AGX_ERR_NULL_POINTER;
    const uint32_t P = plan->num_primes;
    if (q_count == 0 || q_count > AGX_BASIS_MAX_SRC || q_count > P || q_first > P - q_count) return AGX_ERR_BAD_ARGUMENT;
    if (gamma_prime >= P || (gamma_prime >= q_first && gamma_prime - q_first < q_count)) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    return guarded([&]() -> int {
        std::vector<uint64_t> n_inv(q_count), w1n(q_count);
        for (uint32_t i = 0; i < q_count; ++i) n_inv[i] = plan->consts[q_first + i].n_inv, w1n[i] = plan->consts[q_first + i].w1n;
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
    // scratch <- y_i = INTT_i(x_i) gamma t Q_i^-1 mod q_i in [0, q_i): the plan's inverse on the view of Q, its last-stage constants the handle's
    route scaled = prime_range(plan->routes.inverse, cv.q_first, cv.q_first + cv.q_count);
    scaled.consts = h->d_src_consts;
    AGX_HIP(run_inverse(scaled, d_x, nullptr, d_scratch, dense(plan, batch), s));
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
    AGX_HIP(run_inverse(prime_range(plan->routes.inverse, cv.q_first, cv.q_first + cv.q_count), d_x, nullptr, d_scratch, dense(plan, batch), s));
    AGX_HIP(launch_plain_centred_reduce(plan->routes.forward, cv, d_scratch, d_m, f, shoup_quotient(f, cv.t), batch, s));
    return AGX_OK;
}

}  // extern "C"

// ---- agx_ntt_sample_*: ChaCha20 uniform, ternary and binomial sampling (include/agx_ntt.h has the definition, sample_arith.hpp the steps) ----

// One statement of the three calls' rules, the ring calls' in their order: NULL; the range; the frame numbers (frame_first + batch <= 2^32, formed without
// overflow); eta; the form; the plan's device; the pointer and the extent.  The key is HOST memory: its 32 bytes become eight little-endian words of the kernel
// arguments, and nothing of it is kept.  NTT form: the coefficient launch, then the plan's forward on the range in place.
static int sample_call(sample_kind kind, const agx_ntt_plan* plan, const uint8_t* key, uint64_t nonce, uint32_t eta, uint64_t* d_out, uint64_t batch, uint64_t frame_first,
                       uint32_t prime_first, uint32_t prime_count, int out_form, void* stream) {
    if (!plan || !key || !d_out) return AGX_ERR_NULL_POINTER;
    const uint32_t P = plan->num_primes, n = plan->n;
    if (prime_count == 0 || prime_count > P || prime_first > P - prime_count) return AGX_ERR_BAD_ARGUMENT;
    constexpr uint64_t kFrames = (uint64_t)1 << 32;
    if (batch > kFrames || frame_first > kFrames - batch) return AGX_ERR_BAD_ARGUMENT;
    if (kind == SAMPLE_CBD && (eta < 1 || eta > 32)) return AGX_ERR_BAD_ARGUMENT;
    if (out_form != AGX_FORM_COEFF && out_form != AGX_FORM_NTT) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (!aligned8(d_out) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;      // from here on batch n < 2^46
    if (!dense_fits(n, prime_count, batch)) return AGX_ERR_BAD_ARGUMENT;
    if (batch == 0) return AGX_OK;
    uint32_t words[8];
    for (int i = 0; i < 8; ++i) words[i] = (uint32_t)key[4 * i] | (uint32_t)key[4 * i + 1] << 8 | (uint32_t)key[4 * i + 2] << 16 | (uint32_t)key[4 * i + 3] << 24;
    hipStream_t s = static_cast<hipStream_t>(stream);
    AGX_HIP(launch_sample(plan->routes.forward, kind, words, nonce, eta, d_out, batch, frame_first, prime_first, prime_count, s));
    if (out_form == AGX_FORM_NTT) AGX_HIP(run_forward(prime_range(forward_route(plan, batch), prime_first, prime_first + prime_count), d_out, d_out, dense(plan, batch), s));
    return AGX_OK;
}

extern "C" {

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

// ---- agx_ntt_ckks_*: CKKS encoding and decoding (include/agx_ntt.h has the definition, ckks_arith.hpp the per-word steps) ----

// A CKKS boundary on the current device from its image: the buffers, then the view every call hands to its kernel
static int instantiate_ckks(agx_ntt_ckks** out, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count, const ckks_image& img) {
    std::unique_ptr<agx_ntt_ckks> p(new (std::nothrow) agx_ntt_ckks);
    if (!p) return AGX_ERR_ALLOC;
    p->plan = plan;
    static_assert(sizeof(double2) == 2 * sizeof(double), "the twiddle table is uploaded as double2");
    if (int rc = p->d_tw.upload(reinterpret_cast<const double2*>(img.tw.data()), img.tw.size() / 2)) return rc;
    if (int rc = p->d_q.upload(img.q)) return rc;
    if (!img.tri.empty())      // one prime has no Garner constant
        if (int rc = upload_pairs(p->d_tri, img.tri)) return rc;
    if (int rc = upload_pairs(p->d_pow2, img.pow2)) return rc;
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

extern "C" {

// The rules in their order, agx_ntt_plain_create's: NULL; the range; the plan; two equal moduli in the range, a bad modulus.
int agx_ntt_ckks_create(agx_ntt_ckks** h, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count) {
    if (!h) return AGX_ERR_NULL_POINTER;
    *h = nullptr;
    if (!plan) return AGX_ERR_NULL_POINTER;
    const uint32_t P = plan->num_primes;
    if (q_count == 0 || q_count > AGX_BASIS_MAX_SRC || q_count > P || q_first > P - q_count) return AGX_ERR_BAD_ARGUMENT;
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
    if (out_form != AGX_FORM_COEFF && out_form != AGX_FORM_NTT) return AGX_ERR_BAD_ARGUMENT;
    if (int rc = check_plan(plan)) return rc;
    if (!aligned8(d_z) || !aligned8(d_out) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);      // of out ([count][batch][n])
    if (!dense_fits(plan->n, count, batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t slab = batch * plan->n;
    if (ranges_touch(addr(d_z), 2 * batch * slots, addr(d_out), count * slab)) return AGX_ERR_BAD_ARGUMENT;      // a pair of doubles is two words
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    AGX_HIP(launch_ckks_encode(plan->log_n, cv, d_z, (uint32_t)log_s, scale, d_out, batch, count, s));
    // the plan's forward on the view of the call's primes, in place
    if (out_form == AGX_FORM_NTT) AGX_HIP(run_forward(prime_range(forward_route(plan, batch), cv.q_first, cv.q_first + count), d_out, d_out, fl, s));
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
    if (in_form != AGX_FORM_COEFF && in_form != AGX_FORM_NTT) return AGX_ERR_BAD_ARGUMENT;
    const bool ntt = in_form == AGX_FORM_NTT;
    if (int rc = check_plan(plan)) return rc;
    if (!aligned8(d_x) || !aligned8(d_z) || (ntt && !aligned8(d_scratch)) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    const frame_layout fl = dense(plan, batch);      // of x and the scratch ([count][batch][n])
    if (!dense_fits(plan->n, count, batch)) return AGX_ERR_BAD_ARGUMENT;
    const uint64_t words = count * (uint64_t)fl.prime_stride, zwords = 2 * batch * slots;
    // the scratch IS x (the inverse then runs in place) or touches none of it; z touches neither
    if (ntt && d_scratch != d_x && ranges_touch(addr(d_scratch), words, addr(d_x), words)) return AGX_ERR_BAD_ARGUMENT;
    if (ranges_touch(addr(d_z), zwords, addr(d_x), words) || (ntt && ranges_touch(addr(d_z), zwords, addr(d_scratch), words))) return AGX_ERR_BAD_ARGUMENT;
    if (ntt && !plan->has_inverse) return AGX_ERR_NO_INVERSE;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t* coeff = d_x;
    if (ntt) {
        AGX_HIP(run_inverse(prime_range(plan->routes.inverse, cv.q_first, cv.q_first + count), d_x, nullptr, d_scratch, fl, s));
        coeff = d_scratch;
    }
    AGX_HIP(launch_ckks_decode(plan->log_n, cv, coeff, count, scale, d_z, (uint32_t)log_s, batch, s));
    return AGX_OK;
}

int agx_ntt_ckks_twiddle(uint32_t len, uint32_t j, double out[2]) {
    if (!out) return AGX_ERR_NULL_POINTER;
    return ckks_twiddle(len, j, out) ? AGX_OK : AGX_ERR_BAD_ARGUMENT;
}

}  // extern "C"

// ---- agx_ntt_batch_*: SIMD batching of BFV / BGV (include/agx_ntt.h has the definition, batch_arith.hpp the per-word steps, host_math.hpp the tables) ----

agx_ntt_batch::~agx_ntt_batch() { agx::free_plan(plan); }

// the rules the two calls share behind the NULL rule, agx_ntt_plain_*'s order: the plan's device, alignment and the grid limit, the extent
static int batch_call_rules(const agx_ntt_plan* plan, const void* a, const void* b, const void* c, uint64_t batch) {
    if (int rc = check_plan(plan)) return rc;
    if (!aligned8(a) || !aligned8(b) || !aligned8(c) || !batch_fits_grid(plan, batch)) return AGX_ERR_BAD_ARGUMENT;
    return dense_fits(plan->n, 1, batch) ? AGX_OK : AGX_ERR_BAD_ARGUMENT;
}

extern "C" {

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
        if (int rc = agx_ntt_plan_create_auto(&p->plan, n, 1, &t, &img.psi)) return rc;
        if (int rc = p->d_slot_to_word.upload(img.slot_to_word)) return rc;
        if (int rc = p->d_word_to_slot.upload(img.word_to_slot)) return rc;
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
    if (d_scratch != d_m && ranges_touch(addr(d_scratch), words, addr(d_m), words)) return AGX_ERR_BAD_ARGUMENT;
    if (ranges_touch(addr(d_z), words, addr(d_m), words) || ranges_touch(addr(d_z), words, addr(d_scratch), words)) return AGX_ERR_BAD_ARGUMENT;
    if (batch == 0) return AGX_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    AGX_HIP(run_forward(forward_route(plan, batch), d_m, d_scratch, dense(plan, batch), s));
    AGX_HIP(launch_batch_permute(plan->log_n, h->view, false, d_scratch, d_z, batch, s));
    return AGX_OK;
}

}  // extern "C"
