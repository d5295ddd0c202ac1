// ntt_kernels.hpp -- internal launch interface between the C ABI (agx_ntt.cpp) and the
// gfx950 kernels (ntt_kernels.hip).  Not installed; the public surface is include/agx_ntt.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

namespace agx {

struct prime_consts {           // one per prime, device array
    uint64_t q;
    uint64_t mu_hi, mu_lo;      // floor(2^128 / q)           (pointwise multiply)
    uint64_t n_inv, n_inv_p;    // n^-1 mod q and its precomputed quotient      (inverse, last stage)
    uint64_t w1n, w1n_p;        // inv_twiddle[1] * n^-1 mod q and its quotient  (inverse, last stage)
    uint64_t est;               // low word: float slightly below 2^32 / q for reduce_final_est, 0 when q < 2^58;
                                // high word: c when q = 2^60 - c with 0 < c < 2^28, else 0 (reduce_final_q60c, csub_8q_q60c)
};

// agx_ntt_rescale: what prime i < P-1 needs to divide by the last modulus q_L = q_{P-1}; a device array of its own ([P-1]) beside the
// prime_consts, which every kernel loads and which therefore stay as narrow as they are.  q_last and h are the same in every entry.
struct rescale_consts {
    uint64_t qlinv, qlinv_p;    // q_L^-1 mod q_i and its precomputed quotient floor(qlinv * 2^64 / q_i)
    uint64_t h_mod_q;           // h mod q_i, h = (q_L - 1) / 2                  (AGX_RESCALE_ROUND)
    uint64_t q_last, h;
};

// agx_ntt_basis_extend: what a basis (plan, source range, target range) keeps on the device, and its ranges.  S = src_count, T = dst_count.
struct basis_view {
    const ulonglong2* dinv = nullptr;   // [S] {D_i^-1 mod q_i, its precomputed quotient}, q_i the modulus of plan prime src_first + i, D_i = prod_{k != i} q_k
    const ulonglong2* mat = nullptr;    // [T][S] {D_i mod q_j, its precomputed quotient}, q_j the modulus of plan prime dst_first + j
    const ulonglong2* dall = nullptr;   // [T] {D^-1 mod q_j, its precomputed quotient}, D = prod_i q_i (agx_ntt_basis_mod_down; {0, 0} where it does not exist)
    // agx_ntt_basis_mod_down / _mod_down_mode only (null in the view agx_ntt_basis_extend hands out)
    const ulonglong2* down_mat = nullptr;   // [T][S] {t D_i mod q_j, its precomputed quotient}, t the basis' plaintext modulus (1: the words of mat)
    const ulonglong2* round_src = nullptr;  // [S] {c_i = h D_i^-1 mod q_i, q_i}, h = floor(D / 2)                     (AGX_RESCALE_ROUND)
    const uint64_t* round_dst = nullptr;    // [T] t h mod q_j                                                          (AGX_RESCALE_ROUND)
    uint32_t src_first = 0, src_count = 0, dst_first = 0, dst_count = 0;
};

// agx_ntt_basis_extend_exact / _mont: what a basis with an auxiliary prime m keeps beside the above (bfv_conv_arith.hpp has the formulas).  One
// constant set per form, of one shape, so that one kernel body serves both.
struct aux_set {
    const ulonglong2* dinv = nullptr;   // [S] exact: {D_i^-1 mod q_i, quotient} (the words of basis_view::dinv); mont: {m D_i^-1 mod q_i, quotient}
    const ulonglong2* mat = nullptr;    // [T][S] exact: {D_i mod q_j, quotient} (the words of basis_view::mat); mont: {D_i m^-1 mod q_j, quotient}
    const ulonglong2* corr = nullptr;   // [T] exact: {D mod q_j, quotient}; mont: {-D m^-1 mod q_j, quotient}
    uint64_t k = 0, kp = 0;             // exact: D^-1 mod m; mont: -D^-1 mod m; and the quotient
};
struct aux_view {
    const ulonglong2* row = nullptr;    // [S] {D_i mod m, quotient}
    uint64_t m = 0;
    aux_set exact, mont;
};

// agx_ntt_plain_*: what a plaintext boundary (plan, Q = L primes from q_first, the auxiliary prime gamma, the plaintext modulus t) keeps on the device, and
// its scalars (plain_arith.hpp has the formulas).  Every pair is {word, its precomputed quotient for the modulus the word is reduced by}.
struct plain_view {
    const ulonglong2* up = nullptr;      // [L] {t^-1 mod q_i, quotient}                       (scale_up)
    const ulonglong2* one = nullptr;     // [L] {1, floor(2^64 / q_i)}                         (lift)
    const ulonglong2* row_t = nullptr;   // [L] {-q_i^-1 gamma^-1 mod t, quotient}             (scale_down)
    const ulonglong2* row_g = nullptr;   // [L] {-q_i^-1 mod gamma, quotient}                  (scale_down)
    uint64_t t = 0, h = 0, one_p = 0;    // h = floor(t / 2); one_p = floor(2^64 / t): the quotient of the constant 1 modulo t
    uint64_t d = 0, dp = 0;              // D mod t and its quotient
    uint64_t gamma = 0, g = 0, gp = 0;   // gamma; gamma^-1 mod t and its quotient
    uint32_t q_first = 0, q_count = 0;
    // agx_ntt_plain_reduce
    const uint64_t* q = nullptr;         // [L] the moduli of Q
    const ulonglong2* tri = nullptr;     // [L (L - 1) / 2] {q_j^-1 mod q_i, quotient} at i (i - 1) / 2 + j: Garner's constants; null for L = 1
    const ulonglong2* radix_t = nullptr; // [L] {prod_{k < i} q_k mod t, quotient}
};

// agx_ntt_batch_*: what a batching handle (n, t) hands its kernel: the two index tables on the device (host_math.hpp, batch_image) and t's reduction constant
struct batch_view {
    const uint32_t* slot_to_word = nullptr;   // [n] pos(j): decode reads the transformed words through it
    const uint32_t* word_to_slot = nullptr;   // [n] its inverse: encode reads the slots through it
    uint64_t t = 0, one_p = 0;                // one_p = floor(2^64 / t)
};

// agx_ntt_ckks_*: what a CKKS boundary (plan, the primes [q_first, q_first + q_count)) keeps on the device (ckks_arith.hpp has the formulas; host_math.hpp's
// ckks_image says what each table holds).  A call on count <= q_count primes reads a prefix of each.
struct ckks_view {
    const double2* tw = nullptr;         // [n / 2] tw(len, j) at len / 2 + j
    const uint64_t* q = nullptr;         // [q_count]
    const ulonglong2* tri = nullptr;     // [q_count (q_count - 1) / 2] {q_j^-1 mod q_i, quotient} at i (i - 1) / 2 + j
    const ulonglong2* pow2 = nullptr;    // [q_count][1024] {2^e mod q_i, quotient}
    uint32_t q_first = 0, q_count = 0;
};

struct rb_entry;   // one configuration of the kernel registry (rb_registry.hpp): static storage, valid for the life of the library

// device-side view of a plan
struct plan_view {
    uint32_t n = 0, log_n = 0, num_primes = 0;
    const prime_consts* consts = nullptr;  // [P]
    const ulonglong2* tw = nullptr;        // [P][n] {w,w'} natural index   (forward)
    const ulonglong2* itw = nullptr;       // [P][n] {w,w'} natural index   (inverse) or null
    const rb_entry* rb = nullptr;          // the registry entry this view serves, or null (the radix-2 / generic kernels only)
    const ulonglong2* tw_rb = nullptr;     // [P][rb->table_pairs]: the entry's pass tables from the forward tables
    const ulonglong2* itw_rb = nullptr;    // same layout from the inverse tables, or null
    const rescale_consts* rescale = nullptr;   // [P-1], or null (one prime)
    bool q60c_skip = false;                // every modulus of the PLAN is 2^60 - c with 0 < c <= kQ60cSkipMaxC of q60c_class.hpp (so is every range of its primes): an entry
                                           // with a kernel for that class launches it (rb_kernels.hpp: launch_fwd_q60c_skip_t), any other plan gets the entry's general kernel
    // Kernels that hand out frames through a counter ask for a {next frame, retired workgroups} pair of the plan HERE, at launch time and
    // only if they need one: the pair is keyed by the stream (launches on one stream serialise, so they may share a pair; the last
    // workgroup out zeroes it).  nullptr = no pair can be proven free (too many distinct streams): take the stateless fixed-stride form.
    uint32_t* (*ticket_for)(void* ctx, hipStream_t s) = nullptr;
    void (*ticket_launched)(void* ctx, hipStream_t s, uint32_t* pair) = nullptr;      // right behind the launch that uses `pair`: marks when the pair will be idle again
    void* ticket_ctx = nullptr;
    uint32_t* ticket(hipStream_t s) const { return ticket_for ? ticket_for(ticket_ctx, s) : nullptr; }
    void ticket_done(hipStream_t s, uint32_t* pair) const { if (ticket_launched) ticket_launched(ticket_ctx, s, pair); }
};

struct frame_layout {
    uint64_t batch;
    int64_t prime_stride, poly_stride;  // in elements
    bool lazy_out = false;              // forward: results may stay in [0,4q) (kernels are free to reduce fully)
};

// The registry's choice for a plan, made in ONE place (kDefaults / kCompanionDefaults / the `legal` rule, ntt_kernels.hip).
// config_id -1: tuned default for n; arith_level: 0 exact only, 1 every modulus <= 2^61 (fast form legal),
// 2 every modulus <= 2^60 (16q-lazy form legal), 3 every modulus 2^60 - c with 0 < c < 2^28 (the forward kernels specialised for that class)
// narrow_level: 0 some modulus >= 2^31; 1 every modulus < 2^31; 2 every modulus < 2^30 (the 32-bit kernels of rb32_kernels.hpp; they
// also need arith_level >= 1, i.e. tables that honour the precon contract)
struct rb_selection {
    const rb_entry* main = nullptr;            // null: no legal entry (an id of another size or arithmetic class, or none registered)
    const rb_entry* forward_large = nullptr;   // forward-only companion of `main` (a second kernel shape that wins on throughput), its twin for a
                                               // narrower class of moduli already applied; null: none
    uint32_t min_frames = 0;                   // ... for launches of at least this many frames (batch x primes)
};
rb_selection regblock_select(uint32_t n, int config_id, int arith_level, int narrow_level);

hipError_t kernels_init();  // one-time function attributes (large dynamic LDS)

hipError_t launch_forward_radix2(const plan_view& pv, const uint64_t* in, uint64_t* out, const frame_layout& fl, hipStream_t s);
int forward_radix2_launches(uint32_t log_n);      // kernel launches of one launch_forward_radix2 call: the global stages of a frame past the LDS limit, then the LDS kernel
hipError_t launch_inverse_radix2(const plan_view& pv, const uint64_t* in, uint64_t* out, const frame_layout& fl, hipStream_t s);
int inverse_radix2_launches(uint32_t log_n);      // of one launch_inverse_radix2 call: the LDS kernel, then the global stages of a frame past the LDS limit
hipError_t launch_pointwise(const plan_view& pv, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch, hipStream_t s);
// c <- c o bhat in place on the dense [prime][batch][n] layout, bhat with strides of its own as above (the generic path of agx_ntt_polymul_ntt)
hipError_t launch_pointwise_bhat(const plan_view& pv, uint64_t* c, const uint64_t* bhat, uint64_t batch, int64_t bhat_prime_stride,
                                 int64_t bhat_poly_stride, hipStream_t s);
// agx_ntt_inner_product: c_o = sum_t a_t o bhat_{t,o} mod q for `count` primes of the plan in a given order: slot y of the operands is under plan
// prime y for y < split and y + skip behind it (the public call: count = split = P; a key switch below the top level: Q, then the special primes).
struct inner_primes {
    uint32_t count = 0, split = 0, skip = 0;
};
// a dense [terms][count][batch][n], bhat dense [terms][outputs][count][bhat_batch][n] (bhat_batch = batch, or 1: one key frame per prime for every
// frame), c dense [outputs][count][batch][n]; inputs in [0,4q), c in [0,q); out of place (c touches neither input).  pv: a view of the WHOLE plan
// (only its constants are read).  16-byte accesses when all three bases allow them.  terms 1 .. 16, outputs 1 or 2.
// agx_ntt_inner_product_galois: a is read through pi(i) = brev((g brev(i) + (g-1)/2) mod n) within every frame: c_o[i] = sum_t a_t[pi(i)] o bhat_{t,o}[i];
// g odd in [1, 2n).  No permuted copy of a is written.  One launch; g = 1 (agx_ntt_inner_product) takes the un-gathered instance.
hipError_t launch_inner_product_galois(const plan_view& pv, const inner_primes& ip, const uint64_t* a, const uint64_t* bhat, uint64_t* c, uint64_t batch,
                                       uint64_t bhat_batch, uint32_t terms, uint32_t outputs, uint32_t galois_elt, hipStream_t s);
// agx_ntt_add / _sub / _negate / _add_galois / _tensor on the plan primes [first, first + count): every operand set dense [count][batch][n] (the tensor
// product: a, b [2][count][batch][n], c [3][count][batch][n]), slab i under plan prime first + i; inputs in [0,4q), c in [0,q).  pv: a view of the WHOLE
// plan (only its constants are read).  c may be a or b (add, sub), a (negate, add_galois; there c touches b nowhere), neither (tensor; a may be b).
// 16-byte accesses when all bases of the call allow them.  One launch each.  The linear calls: c = a + b[pi_g], a - b or -a (which reads no b: pass a); g is 1
// but for add_galois, where g = 1 takes the plain add's instance.
enum ring_op { RING_ADD, RING_SUB, RING_NEG };
hipError_t launch_ring_linear(const plan_view& pv, uint32_t first, uint32_t count, ring_op op, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch,
                              uint32_t galois_elt, hipStream_t s);
hipError_t launch_ring_tensor(const plan_view& pv, uint32_t first, uint32_t count, const uint64_t* a, const uint64_t* b, uint64_t* c, uint64_t batch, hipStream_t s);
// agx_ntt_mul_add_galois: c[i] = (accumulate ? c[i] : 0) + w[i] o b[pi_g(i)] over the same range; w is [count][w_batch][n], w_batch = batch or 1 (one
// frame per prime for every frame of the batch).  One launch; g = 1 takes the un-gathered instance.
hipError_t launch_ring_mul_add_galois(const plan_view& pv, uint32_t first, uint32_t count, const uint64_t* w, uint64_t w_batch, const uint64_t* b, uint64_t* c,
                                      uint64_t batch, uint32_t galois_elt, bool accumulate, hipStream_t s);
// agx_ntt_keyswitch_accumulate_decomposed: launch_inner_product_galois with two outputs and a broadcast key, then acc_o = (accumulate ? acc_o : 0) +
// weight o (the sum) per word; weight [ip.count][weight_batch][n] or nullptr (w = 1).  One launch; g = 1 takes the un-gathered instance.
hipError_t launch_inner_weighted(const plan_view& pv, const inner_primes& ip, const uint64_t* a, const uint64_t* bhat, const uint64_t* weight, uint64_t weight_batch,
                                 uint64_t* acc, uint64_t batch, uint32_t terms, uint32_t galois_elt, bool accumulate, hipStream_t s);
// the coefficient-domain step of agx_ntt_rescale's generic route: out_i[k] <- (out_i[k] - u_i[k]) q_L^-1 mod q_i on the dense [prime][batch][n]
// layout of pv's primes (a view of primes 0 .. P-2), u_i the lift of t[k] ([batch][n], coefficients of the last slab in [0, q_L)) to q_i
hipError_t launch_rescale_coeff(const plan_view& pv, uint64_t* out, const uint64_t* t, uint64_t batch, bool round, hipStream_t s);
// agx_ntt_automorphism on the dense [prime][batch][n] layout of pv's primes, out of place (the ranges must not touch), g odd in [1, 2n).
// NTT form: a permutation of words, the modulus is not read; 16-byte accesses when both bases allow them.  Coefficient form: inputs in
// [0,4q), outputs in [0,q); gathered from global memory (the stride-g^-1 repeats hit L2).  One launch each.
hipError_t launch_automorphism_ntt(const plan_view& pv, const uint64_t* in, uint64_t* out, uint64_t batch, uint32_t g, hipStream_t s);
hipError_t launch_automorphism_coeff(const plan_view& pv, const uint64_t* in, uint64_t* out, uint64_t batch, uint32_t g, hipStream_t s);
// agx_ntt_basis_extend in coefficient form: x dense [S][batch][n] (slab i under plan prime src_first + i, values in [0,4q_i)) -> out dense
// [T][batch][n] (slab j under plan prime dst_first + j), out_j = sum_i y_i (D_i mod q_j) mod q_j in [0,q_j), y_i = x_i D_i^-1 mod q_i in [0,q_i).
// pv: a view of the WHOLE plan (only its constants are read); out of place (the ranges must not touch).  One launch.
hipError_t launch_basis_coeff(const plan_view& pv, const basis_view& bv, const uint64_t* x, uint64_t* out, uint64_t batch, hipStream_t s);
// agx_ntt_basis_extend_exact (exact: xaux dense [1][batch][n] under the auxiliary prime, values in [0,4m)) and agx_ntt_basis_extend_mont (xaux is not read)
// in coefficient form: x and out as launch_basis_coeff takes them, out fully reduced; out touches neither input.  One launch.
hipError_t launch_basis_aux_coeff(const plan_view& pv, const basis_view& bv, const aux_view& av, bool exact, const uint64_t* x, const uint64_t* xaux, uint64_t* out,
                                  uint64_t batch, hipStream_t s);
// the coefficient-domain step of agx_ntt_basis_quotient on a basis with sources B (S = K), targets Q (T = L) and the auxiliary prime m: y dense
// [T + S + 1][batch][n] as the scaled inverses left it -- the y_i in [0,q_i) under Q, then the s_j in [0,b_j) under B, then s_m in [0,m) -- and qmat [T][S + 1]
// {q_i^-1 B_j^-1 mod b_j, quotient}, column S {q_i^-1 mod m, quotient} -> out dense [T][batch][n] in coefficient form, fully reduced
// (bfv_quotient_arith.hpp).  The return reads the exact conversion's constants of av.  pv: a view of the WHOLE plan (only its constants are read); out
// touches y nowhere.  One launch.
hipError_t launch_basis_quotient(const plan_view& pv, const basis_view& bv, const aux_view& av, const ulonglong2* qmat, const uint64_t* y, uint64_t* out, uint64_t batch,
                                 hipStream_t s);
// the coefficient-domain step of agx_ntt_basis_mod_down's generic route: out_j[k] <- (out_j[k] - sum_i y_i[k] (D_i mod q_j)) D^-1 mod q_j in place on
// out, dense [T][batch][n] in coefficient form with values in [0,q_j) (slab j under plan prime dst_first + j); y: dense [S][batch][n], y_i in
// [0,q_i) as the scaled inverse of the source slabs left them.  pv: a view of the WHOLE plan (only its constants are read).  One launch.  The matrix is
// bv.down_mat; round: AGX_RESCALE_ROUND, with bv.round_src and bv.round_dst (moddown_arith.hpp).
hipError_t launch_moddown_coeff(const plan_view& pv, const basis_view& bv, uint64_t* out, const uint64_t* y, uint64_t batch, bool round, hipStream_t s);
// agx_ntt_plain_scale_up (lift = false) and agx_ntt_plain_lift in coefficient form: m dense [batch][n], any words -> out dense [L][batch][n], slab i under
// plan prime q_first + i, fully reduced (plain_arith.hpp).  pv: a view of the WHOLE plan (only its constants are read); out touches m nowhere.  One launch.
hipError_t launch_plain_encode(const plan_view& pv, const plain_view& cv, bool lift, const uint64_t* m, uint64_t* out, uint64_t batch, hipStream_t s);
// the coefficient-domain step of agx_ntt_plain_scale_down: y dense [L][batch][n], y_i in [0, q_i) as the scaled inverse of the Q slabs left them -> m dense
// [batch][n] in [0, t).  m touches y nowhere.  One launch.
hipError_t launch_plain_scale_down(const plan_view& pv, const plain_view& cv, const uint64_t* y, uint64_t* m, uint64_t batch, hipStream_t s);
// agx_ntt_ckks_encode in coefficient form: z dense [batch][2^log_s] pairs of doubles -> out dense [count][batch][n], slab i under plan prime q_first + i, fully
// reduced; out touches z nowhere.  One launch, one workgroup per frame (ckks_kernels.hpp); log_s <= log_n - 1.
hipError_t launch_ckks_encode(uint32_t log_n, const ckks_view& cv, const double* z, uint32_t log_s, double scale, uint64_t* out, uint64_t batch, uint32_t count, hipStream_t s);
// agx_ntt_ckks_decode behind the inverse: x dense [count][batch][n], fully reduced -> z dense [batch][2^log_s] pairs; z touches x nowhere.  One launch.
hipError_t launch_ckks_decode(uint32_t log_n, const ckks_view& cv, const uint64_t* x, uint32_t count, double scale, double* z, uint32_t log_s, uint64_t batch, hipStream_t s);
// agx_ntt_sample_uniform / _ternary / _cbd in coefficient form: out dense [count][batch][n], slab i under plan prime first + i, fully reduced; frame f of
// the launch is frame frame_first + f of the draw (frame_first + batch <= 2^32).  key: the eight little-endian words of the caller's 32 bytes, copied into
// the kernel arguments.  pv: a view of the WHOLE plan (only its constants are read).  One launch each; the 16-byte stores when out allows them.
enum sample_kind { SAMPLE_UNIFORM, SAMPLE_TERNARY, SAMPLE_CBD };
hipError_t launch_sample(const plan_view& pv, sample_kind kind, const uint32_t key[8], uint64_t nonce, uint32_t eta, uint64_t* out, uint64_t batch, uint64_t frame_first,
                         uint32_t first, uint32_t count, hipStream_t s);
// the coefficient-domain step of agx_ntt_plain_reduce: y dense [L][batch][n], y_i in [0, q_i) as the plan's inverse of the Q slabs left them -> m dense
// [batch][n] = f X mod t in [0, t), X the centred representative, f < t with its quotient fp.  m touches y nowhere.  One launch.
hipError_t launch_plain_centred_reduce(const plan_view& pv, const plain_view& cv, const uint64_t* y, uint64_t* m, uint64_t f, uint64_t fp, uint64_t batch, hipStream_t s);
// the permutation of agx_ntt_batch_encode (encode = true: out[frame][w] = in[frame][word_to_slot[w]] mod t, any words in) and agx_ntt_batch_decode (out[frame][j]
// = in[frame][slot_to_word[j]], moved as they are) on dense [batch][n] words; out touches in nowhere.  One launch; 16-byte stores when out is 16-byte aligned.
hipError_t launch_batch_permute(uint32_t log_n, const batch_view& bv, bool encode, const uint64_t* in, uint64_t* out, uint64_t batch, hipStream_t s);
hipError_t launch_fill(const plan_view& pv, uint64_t* out, uint64_t batch, uint64_t first_poly, uint64_t seed, hipStream_t s);

}  // namespace agx
