/*
 * agx_ntt.h -- C ABI of the MI355X-native batched negacyclic NTT engine.
 *
 * This is the drop-in boundary for the forward-NTT path of joekurina/Agilex-NTT
 * (reference paths are relative to the reference tree).  Everything is plain
 * pointers and sizes: no SYCL, HIP or torch types appear in a signature
 * (streams are passed as `void*` holding a hipStream_t; NULL = default stream).
 *
 * Data contract (verified against the reference arithmetic):
 *   one "frame" = one length-n polynomial under one modulus q, n a power of two,
 *   q prime, q = 1 (mod 2n), q < 2^62, coefficients uint64_t.
 *   forward : out[bitrev(k)] = sum_j x[j] * psi^((2k+1) j) mod q, fully reduced to [0,q)
 *             (natural order in, bit-reversed order out; inputs may lie in [0,4q)).
 *   inverse : exact inverse of forward (bit-reversed in, natural out, [0,q)).
 *   tables  : twiddle[j] = psi^bitrev(j) mod q,  precon[j] = floor(twiddle[j] * 2^64 / q),
 *             j = 0..n-1 (index 0 unused by the transform), as the reference expects
 *             its caller to supply them (include/kernel/ntt.h:35-41).
 *
 * Every function returns an agx_status (0 = success) and never throws.
 */
#ifndef AGX_NTT_H
#define AGX_NTT_H

#include <stddef.h>
#include <stdint.h>

/* the library is built with -fvisibility=hidden: only the entry points declared here are exported */
#if defined(__GNUC__) || defined(__clang__)
#define AGX_API __attribute__((visibility("default")))
#else
#define AGX_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum agx_status {
    AGX_OK = 0,
    AGX_ERR_NULL_POINTER = 1,   /* a required pointer argument is NULL                      */
    AGX_ERR_BAD_SIZE = 2,       /* n is not a power of two in [AGX_NTT_MIN_N, AGX_NTT_MAX_N] */
    AGX_ERR_BAD_MODULUS = 3,    /* q >= 2^62, q even, q != 1 (mod 2n) or (plan_create_auto) q composite; rescale: q_i == q_last; mod_down: a target modulus equal to a source modulus; keyswitch_create: two equal active moduli */
    AGX_ERR_BAD_ROOT = 4,       /* psi is not a primitive 2n-th root of unity mod q           */
    AGX_ERR_BAD_ARGUMENT = 5,   /* zero primes, negative stride, a layout extent past 2^60 words, overlapping in/out, an even or too large Galois element, an unknown form or mode, a term, output or digit count out of range, ... */
    AGX_ERR_NO_DEVICE = 6,      /* no usable HIP device                                       */
    AGX_ERR_HIP = 7,            /* a HIP runtime call failed (agx_ntt_last_hip_error)         */
    AGX_ERR_ALLOC = 8,          /* host or device allocation failed                           */
    AGX_ERR_NO_INVERSE = 9      /* plan was created without inverse tables                    */
} agx_status;

#define AGX_NTT_MIN_N 2u
#define AGX_NTT_MAX_N 32768u  /* the reference's largest size (include/kernel/ntt.h:19-20) */

/* kernel variants (agx_ntt_plan_set_variant); AUTO picks the tuned kernel for n */
#define AGX_VARIANT_AUTO 0
#define AGX_VARIANT_LDS_RADIX2 1 /* one stage per barrier, LDS resident: mirrors the reference's op sequence */
#define AGX_VARIANT_REGBLOCK 2   /* register-blocked radix-2^R passes, tuned configuration for n */
#define AGX_VARIANT_REGBLOCK_BASE 256 /* + k: k-th entry of the kernel registry (A/B measurements only) */

AGX_API const char* agx_ntt_strerror(int status);
AGX_API int agx_ntt_last_hip_error(void);     /* hipError_t of the last AGX_ERR_HIP on this thread */
AGX_API int agx_ntt_device_count(int* count); /* AGX_OK and *count = 0 when there is no GPU */

/* ------------------------------------------------------------------------- */
/* (1) One-shot host-pointer forward NTT.                                     */
/* Replaces the reference's three calls taken together:                        */
/*   ntt_input_kernel(inData, inData2, modulus, twiddleFactors,                */
/*                    barrettTwiddleFactors, numFrames, q)  include/kernel/ntt.h:35-41 */
/*   fwd_ntt_kernel<0>(q)                                   include/kernel/ntt.h:32-33 */
/*   ntt_output_kernel(outData, numFrames, q)               include/kernel/ntt.h:43-45 */
/* Reads only in[b*n + 0 .. n/2) and in2[b*n + n/2 .. n) (src/kernel/ntt.cpp:584-590; */
/* in2 may alias in), writes out[b*n + p] (src/kernel/ntt.cpp:628-633).  n is a */
/* runtime argument here (the reference fixes it at compile time,              */
/* include/kernel/ntt.h:7-23).  Synchronous; all pointers are host memory.     */
/* ------------------------------------------------------------------------- */
/* With AGX_NTT_DEVICES=0,1,2,3 in the environment the frames are dealt to those devices in contiguous blocks (a group, section 5) instead */
/* of running on the current one: the reference's NUM_NTT_COMPUTE_UNITS replication (src/kernel/ntt.cpp:8-12, 526-536) for a caller that  */
/* cannot change its code; a device id that does not exist returns AGX_ERR_BAD_ARGUMENT.                                                  */
AGX_API int agx_ntt_forward_host(const uint64_t* in, const uint64_t* in2, const uint64_t* modulus,
                         const uint64_t* twiddles, const uint64_t* precons, uint64_t* out,
                         uint32_t n, uint32_t num_frames);

/* The same path for repeated calls and large inputs: tables stay on the device in `plan` (one modulus) */
/* and host frames stream through pinned staging buffers with upload, transform and download          */
/* overlapped on three HIP streams (the reference streams frames through its input/output kernels,    */
/* src/kernel/ntt.cpp:508-640).  agx_ntt_forward_host is this call on a plan it builds from the caller's */
/* tables and keeps for the next call with the same (n, modulus, tables).                              */
struct agx_ntt_plan;
AGX_API int agx_ntt_forward_host_stream(const struct agx_ntt_plan* plan, const uint64_t* in, const uint64_t* in2,
                                uint64_t* out, uint64_t num_frames);
/* the inverse transform through the same pipeline (bit-reversed order in, natural order out, one modulus; the reference ships no */
/* inverse path -- SURVEY F2 -- so there is no operand pairing to mirror)                                                         */
AGX_API int agx_ntt_inverse_host_stream(const struct agx_ntt_plan* plan, const uint64_t* in, uint64_t* out, uint64_t num_frames);

/* Releases what the library keeps between calls: the one-shot plan of every device (agx_ntt_forward_host keeps the plan of its */
/* last call per device) and the per-device pool of pinned / device staging buffers of the streaming path (192 MiB pinned +     */
/* 96 MiB device memory per device that has used it).  Call before hipDeviceReset and at shutdown; later calls rebuild on demand. */
/* (The reference holds its buffers in SYCL RAII objects of main(), src/main.cpp:32-37; this is the explicit counterpart.)       */
AGX_API int agx_ntt_release_caches(void);

/* ------------------------------------------------------------------------- */
/* (2) Plans: device-resident tables for num_primes moduli of one size n.      */
/* A plan is immutable after creation and may be shared between host threads   */
/* and streams (kernels that hand out frames through a counter keep one counter */
/* pair per stream, for up to 64 distinct streams per plan; launches on further */
/* streams -- and on hipStreamPerThread, one handle that names a different      */
/* stream in every host thread -- take a stateless kernel form: slower by a few */
/* per cent, never wrong);                                                       */
/* it belongs to the HIP device that was current when it was created: calls    */
/* that take it return AGX_ERR_BAD_ARGUMENT while another device is current.   */
/* ------------------------------------------------------------------------- */
typedef struct agx_ntt_plan agx_ntt_plan;

/* caller-supplied tables, laid out [num_primes][n] (one reference launch per prime,
 * src/kernel/ntt.cpp:143-144,569).  inv_* may both be NULL (forward-only plan).
 * n_inv[p] = n^-1 mod q_p is derived internally. */
AGX_API int agx_ntt_plan_create(agx_ntt_plan** plan, uint32_t n, uint32_t num_primes, const uint64_t* moduli,
                        const uint64_t* twiddles, const uint64_t* precons,
                        const uint64_t* inv_twiddles, const uint64_t* inv_precons);

/* tables generated by the library; psi == NULL -> smallest primitive 2n-th root per prime */
AGX_API int agx_ntt_plan_create_auto(agx_ntt_plan** plan, uint32_t n, uint32_t num_primes,
                             const uint64_t* moduli, const uint64_t* psi);
AGX_API int agx_ntt_plan_destroy(agx_ntt_plan* plan);
/* testing / benchmarking only.  NOT thread-safe: it rebuilds the plan's pass tables, so no launch that uses the plan may be in flight */
/* or be issued from another thread while it runs (it synchronises the device before it frees the old tables)                         */
AGX_API int agx_ntt_plan_set_variant(agx_ntt_plan* plan, int variant);
AGX_API int agx_ntt_plan_info(const agx_ntt_plan* plan, uint32_t* n, uint32_t* num_primes, int* device, int* has_inverse);
/* which kernel a forward call of `batch` frames per prime runs: its id in the kernel registry (the k of AGX_VARIANT_REGBLOCK_BASE + k), -1 for */
/* the LDS radix-2 kernels.  Read-only; for tests and A/B measurements                                                                       */
AGX_API int agx_ntt_plan_forward_kernel(const agx_ntt_plan* plan, uint64_t batch, int* registry_id);
AGX_API int agx_ntt_plan_get_modulus(const agx_ntt_plan* plan, uint32_t prime_index, uint64_t* q, uint64_t* psi);

/* ------------------------------------------------------------------------- */
/* (3) Device-pointer batched transforms.  Frame (p, b) starts at              */
/* base + p*prime_stride + b*poly_stride (strides in uint64_t elements);       */
/* the dense forms use the [prime][batch][n] layout (prime_stride = batch*n,   */
/* poly_stride = n).  Base pointers need 8-byte alignment only (frames need    */
/* not start on a 16-byte boundary), and strides may be odd.                   */
/* In place (d_out == d_in) is allowed; an output whose                        */
/* frames touch the input's frames without being the same frames (d_out =      */
/* d_in + n/2, c = a + 8 ...) returns AGX_ERR_BAD_ARGUMENT: workgroups run in  */
/* any order, so such a call would corrupt its own inputs.  A layout whose     */
/* own frames touch one another (two distinct (p, b) less than n elements      */
/* apart: prime_stride = 0 with two primes, prime_stride = poly_stride = n     */
/* with two polynomials, ...) returns AGX_ERR_BAD_ARGUMENT too: two workgroups */
/* would transform the same words under different moduli.  So does a layout    */
/* whose extent (P-1)*prime_stride + (B-1)*poly_stride + n is more than 2^60   */
/* words: its byte offsets would not fit 64 bits.  Asynchronous on             */
/* `stream`; nothing is allocated or synchronised inside, so the calls can be  */
/* captured into a hipGraph (kernels that hand out frames through a counter    */
/* switch to a stateless form while the stream is capturing).                   */
/* ------------------------------------------------------------------------- */
AGX_API int agx_ntt_forward(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, void* stream);
AGX_API int agx_ntt_inverse(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, void* stream);
/* forward with HEXL-style lazy outputs: results are congruent to the transform and lie in [0,4q)
 * (the last two conditional subtracts of src/kernel/ntt.cpp:377-394 are skipped where that saves
 * work); agx_ntt_inverse, agx_ntt_pointwise and agx_ntt_forward all accept such values as inputs */
AGX_API int agx_ntt_forward_lazy(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, void* stream);
AGX_API int agx_ntt_forward_strided(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch,
                            int64_t prime_stride, int64_t poly_stride, void* stream);
AGX_API int agx_ntt_inverse_strided(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch,
                            int64_t prime_stride, int64_t poly_stride, void* stream);
/* agx_ntt_forward / agx_ntt_inverse on the plan primes [prime_first, prime_first + prime_count), the range convention of the ring calls below: d_in and
 * d_out dense [prime_count][batch][n], slab i under plan prime prime_first + i.  The words are exactly what a plan over those primes with the same roots
 * would write, so no second plan is needed to transform the Q slabs of a ciphertext on a plan that also carries special or auxiliary primes; over
 * (0, P) the calls are agx_ntt_forward / agx_ntt_inverse word for word and launch their kernels.  In place is allowed.  Rules: those of agx_ntt_forward /
 * agx_ntt_inverse in their order (the frames are the range's), with the range rule right behind the NULL rule: prime_count == 0 or a range past P:
 * AGX_ERR_BAD_ARGUMENT, nothing written.  Route: the plan's own route for this batch, viewed on the range (the views the RNS calls run internally): no new
 * kernel, the launch counts of the whole-plan calls, capturable as they are. */
AGX_API int agx_ntt_forward_range(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t prime_first, uint32_t prime_count,
                                  void* stream);
AGX_API int agx_ntt_inverse_range(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t prime_first, uint32_t prime_count,
                                  void* stream);

/* c = a o b (coefficient-wise product mod q_p), dense [prime][batch][n] layout; c may alias a or b */
AGX_API int agx_ntt_pointwise(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c,
                      uint64_t batch, void* stream);
/* c = a * b in Z_q[X]/(X^n + 1) = INTT(NTT(a) o NTT(b)); dense layout; c may alias a, b or both (squaring in place: a == b == c).
 * d_scratch: num_primes*batch*n elements of device memory owned by the caller, disjoint from a, b, c.
 * Every size has a one-launch fused kernel, so d_scratch may be NULL; it is only used by plans forced onto the radix-2
 * kernels (AGX_VARIANT_LDS_RADIX2: three launches), where a NULL scratch returns AGX_ERR_NULL_POINTER. */
AGX_API int agx_ntt_polymul(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c,
                    uint64_t* d_scratch, uint64_t batch, void* stream);

/* c = a * b in Z_q[X]/(X^n + 1) with b given by its transform: d_bhat holds what agx_ntt_forward or agx_ntt_forward_lazy
 * OF THIS PLAN wrote for b (bit-reversed order; values in [0,q), or lazy exactly as agx_ntt_forward_lazy leaves them): the
 * product for a fixed operand (a key, a plaintext, a gadget row) that the caller keeps in NTT form -- two transforms
 * instead of the three of agx_ntt_polymul.
 * a, c: dense [prime][batch][n].  d_bhat: dense [prime][bhat_batch][n] with bhat_batch == batch (frame (p, f) is
 * multiplied by bhat frame (p, f)) or bhat_batch == 1 (every frame of prime p is multiplied by the one bhat frame (p, 0):
 * the shared operand is stored and fetched once, 16n + 8n/batch bytes of traffic per product instead of 24n).
 * a may hold values in [0,4q) wherever agx_ntt_polymul accepts them; c is fully reduced.  c may alias a (in place);
 * c must not touch d_bhat, and c / a must not partially overlap: AGX_ERR_BAD_ARGUMENT, nothing written.  bhat_batch other
 * than batch or 1: AGX_ERR_BAD_ARGUMENT; a plan without inverse tables: AGX_ERR_NO_INVERSE.
 * Asynchronous on `stream`, allocates and synchronises nothing (capturable into a hipGraph), needs no scratch.
 * ONE launch (forward, product with bhat as it streams in, inverse, one frame on chip) for n = 1024 ... 32768 whenever some
 * modulus is 2^31 or larger (the 16q-lazy, fast and exact 64-bit kernels alike).  Three launches (forward a -> c, c o bhat in
 * place, inverse c -> c; 40n bytes) for n <= 512, for plans whose moduli are all below 2^31 (the 32-bit kernels) and for
 * plans forced onto AGX_VARIANT_LDS_RADIX2. */
AGX_API int agx_ntt_polymul_ntt(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_bhat, uint64_t* d_c,
                                uint64_t batch, uint64_t bhat_batch, void* stream);

/* Exact division by the plan's LAST modulus q_L = q_{P-1} on NTT-form frames, P >= 2: the CKKS "rescale" and the BFV form of modulus switching.
 * It takes no plaintext modulus t, so it is NOT the BGV modulus switch, which must keep the value modulo t: that is agx_ntt_basis_create_plain with
 * agx_ntt_basis_mod_down_mode below, which also rounds at any level of one plan (this call divides by the plan's last prime only).
 * Per coefficient, with X in [0, q_0 ... q_{P-1}) the integer the P residues represent and h = (q_L - 1) / 2:
 *   AGX_RESCALE_FLOOR: Y = floor(X / q_L)         AGX_RESCALE_ROUND: Y = floor((X + h) / q_L)
 * and out holds Y mod q_i for i < P-1, fully reduced.  Input and output are in NTT form (bit-reversed order, as agx_ntt_forward of this
 * plan writes it); no approximation anywhere: t = INTT_L(x_L) (+ h mod q_L), out_i = (x_i - NTT_i(t mod q_i - h mod q_i)) q_L^-1 mod q_i.
 * d_x: dense [P][batch][n], values in [0,q) or lazy exactly as agx_ntt_forward_lazy leaves them.  d_out: dense [P-1][batch][n].
 * d_scratch: batch*n elements of device memory; it receives the coefficient form of the last slab.
 * Aliasing: d_out == d_x is allowed (in place: slabs 0 .. P-2 of both coincide).  d_scratch may be exactly d_x's last slab,
 * d_x + (P-1)*batch*n: the caller thereby GIVES THAT SLAB UP (it is overwritten) -- with d_out == d_x this is the in-place use, which
 * needs no memory beyond x.  Otherwise d_scratch must be disjoint from d_x and d_out, and x is left unchanged.  d_out partially overlapping
 * d_x, d_out touching the scratch, or the scratch touching slabs 0 .. P-2 of d_x: AGX_ERR_BAD_ARGUMENT, nothing written.
 * One prime, or a mode other than the two above: AGX_ERR_BAD_ARGUMENT; a modulus q_i, i < P-1, equal to q_L (decided at the call: plan
 * creation accepts such plans): AGX_ERR_BAD_MODULUS; a plan without inverse tables: AGX_ERR_NO_INVERSE.
 * Asynchronous on `stream`, allocates and synchronises nothing (capturable into a hipGraph).
 * TWO launches (the inverse of the last slab into the scratch; then, one frame on chip, the lift to q_i, the forward transform and the
 * difference with x_i as it streams in) for n = 1024 ... 32768 whenever some modulus is 2^31 or larger.  Four (inverse of slabs 0 .. P-2
 * into out, inverse of the last slab, one coefficient-domain pass over out, forward of out in place) for n <= 512, for plans whose moduli
 * are all below 2^31 and for plans forced onto AGX_VARIANT_LDS_RADIX2. */
#define AGX_RESCALE_FLOOR 0
#define AGX_RESCALE_ROUND 1
AGX_API int agx_ntt_rescale(const agx_ntt_plan* plan, const uint64_t* d_x, uint64_t* d_out, uint64_t* d_scratch,
                            uint64_t batch, int mode, void* stream);

/* The Galois automorphism sigma_g: a(X) -> a(X^g) mod (X^n + 1), g = galois_elt odd, 1 <= g < 2n, on every frame of the dense [prime][batch][n]
 * layout: the ring operation of every CKKS / BGV slot rotation (g = 5^step mod 2n, agx_ntt_galois_element) and of conjugation (g = 2n - 1).
 *   AGX_FORM_COEFF (natural order): coefficient j goes to position e = g j mod 2n if e < n, and negated to position e - n otherwise; inputs may lie
 *     in [0,4q) as agx_ntt_forward accepts them, outputs are fully reduced (so -0 = 0).  g = 1 is a reduce-to-[0,q) copy.
 *   AGX_FORM_NTT (bit-reversed order, as agx_ntt_forward / agx_ntt_forward_lazy of this plan write it): out[p] = in[brev((g brev(p) + (g-1)/2) mod n)],
 *     brev the log2(n)-bit reversal: a pure permutation of 64-bit words.  No arithmetic and no modulus: lazy values stay exactly as they were.
 *     g = 1 is a copy.  agx_ntt_inverse of the result is the AGX_FORM_COEFF result of the coefficients.
 * Every plan serves both forms, whatever its variant or moduli; no inverse tables are needed.  No tables of its own either: plan creation is unchanged.
 * OUT OF PLACE ONLY: d_out's [prime][batch][n] range may not touch d_in's anywhere, equal pointers included (AGX_ERR_BAD_ARGUMENT, nothing written):
 * workgroups run in any order and a frame is permuted across its whole length, so no workgroup could read all it needs before another has
 * written there.  galois_elt even or >= 2n, or a form other than the two below: AGX_ERR_BAD_ARGUMENT.  Pointers need 8-byte alignment only.
 * Asynchronous on `stream`, allocates and synchronises nothing, touches no plan state (capturable into a hipGraph).  ONE launch in either form:
 * NTT form one thread per word (per pair of words with 16-byte accesses when both bases are 16-byte aligned), no LDS, no barrier -- a wave
 * that writes 64 consecutive words reads one 512-byte segment; coefficient form one thread per word, gathered from global memory (the repeats hit L2).
 * Either form runs at the rate of a device copy of the same words or above it (profiles/r07_automorphism.md). */
#define AGX_FORM_COEFF 0
#define AGX_FORM_NTT 1
AGX_API int agx_ntt_automorphism(const agx_ntt_plan* plan, const uint64_t* d_in, uint64_t* d_out, uint64_t batch, uint32_t galois_elt, int form,
                                 void* stream);

/* Fast RNS base conversion ("fast basis extension", HPS / BEHZ): a polynomial known by its residues modulo the SOURCE primes [src_first, src_first + S)
 * of a plan gets its residues modulo the TARGET primes [dst_first, dst_first + T): both halves of a hybrid key switch -- ModUp extends one digit to the
 * whole basis Q u P, ModDown brings the special primes back to Q.  Both ranges lie inside the plan's primes [0, P); they may overlap,
 * or one may contain the other.  Per coefficient, with D = prod_{i in source} q_i and D_i = D / q_i:
 *   y_i = (x_i mod q_i) (D_i^-1 mod q_i) mod q_i in [0, q_i),    V = sum_i y_i D_i (an integer, 0 <= V < S D),    out_j = V mod q_j, fully reduced.
 * This is the APPROXIMATE conversion: V = X + u D with X in [0, D) the CRT value of the residues and 0 <= u < S; no correction term is applied, callers
 * absorb u D in their noise, as every hybrid key switch does.  It is a deterministic integer formula (exact against big-integer arithmetic); for a
 * target j that is itself a source prime it gives out_j = x_j mod q_j.
 * A BASIS holds the constants of one (plan, ranges) on the plan's device -- D_i^-1 mod q_i (S entries) and D_i mod q_j (T x S), computed once on the
 * host -- and a pointer to the plan, nothing else of it: agx_ntt_plan_set_variant between calls stays legal, the plan must outlive the basis, and the
 * plan's device must be current at creation and at every call.  Any plan serves (no inverse tables needed); plan creation is unchanged.
 * S <= AGX_BASIS_MAX_SRC = 16 is part of the contract: it is what lets sum_i y_i (D_i mod q_j) < 16 2^62 2^62 = 2^128 be kept unreduced in 128 bits.
 * (The kernels here reduce every term lazily instead and keep one 64-bit accumulator per coefficient.)
 *   create : NULL basis or plan: AGX_ERR_NULL_POINTER; src_count == 0, dst_count == 0, a range past P, src_count > 16: AGX_ERR_BAD_ARGUMENT; two equal
 *            source moduli (D_i is not invertible modulo q_i): AGX_ERR_BAD_MODULUS.        destroy: NULL is fine.
 *   info   : the ranges, and launches_ntt_form = the kernel launches an AGX_FORM_NTT call takes under the plan's CURRENT variant.  Any out-pointer may be NULL.
 *   extend : d_x dense [S][batch][n], COEFFICIENT form (natural order), slab i under prime src_first + i, values in [0, 4 q_i) as agx_ntt_forward accepts them;
 *            d_out dense [T][batch][n], slab j under prime dst_first + j.  out_form AGX_FORM_COEFF writes out_j as defined above; AGX_FORM_NTT writes
 *            NTT_j(out_j) exactly as agx_ntt_forward of this plan would write it (bit-reversed order, fully reduced).  Pointers need 8-byte alignment only.
 *            OUT OF PLACE ONLY: d_out's range may not touch d_x's anywhere (AGX_ERR_BAD_ARGUMENT, nothing written).  An unknown form: AGX_ERR_BAD_ARGUMENT;
 *            batch == 0: AGX_OK, nothing launched.  Asynchronous on `stream`, allocates and synchronises nothing (capturable into a hipGraph).
 * AGX_FORM_COEFF is ONE launch on every plan (one thread per coefficient: S words read, T written, 8n(S + T) bytes per frame).  AGX_FORM_NTT is ONE launch
 * (the conversion into one target prime's frame on chip, its forward transform, the store; T workgroups per frame) for n = 1024 ... 32768 whenever some modulus is
 * 2^31 or larger AND the source count is one at which that kernel measured ahead of the two-launch form (profiles/r08_basis_extend.md): S = 1, and S = 2 except at
 * n = 4096 and 16384; there T ceil(batch / frames per workgroup) workgroups past 2^31 - 1 return AGX_ERR_BAD_ARGUMENT.  Everywhere else -- S >= 3, S = 2 at n = 4096
 * and 16384, n <= 512, plans whose moduli are all below 2^31, plans forced onto AGX_VARIANT_LDS_RADIX2 -- it is the coefficient-form launch followed by the plan's
 * forward on the target slabs in place (two launches; three at n = 32768 under AGX_VARIANT_LDS_RADIX2, whose forward is two).
 * Groups: there is no group form.  A basis is tied to one plan; agx_ntt_group_shard hands out each shard's plan and stream, so a caller makes one
 * basis per shard and calls agx_ntt_basis_extend on that shard's device and stream. */
#define AGX_BASIS_MAX_SRC 16
typedef struct agx_ntt_basis agx_ntt_basis;
AGX_API int agx_ntt_basis_create(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count);
AGX_API int agx_ntt_basis_destroy(agx_ntt_basis* basis);
AGX_API int agx_ntt_basis_info(const agx_ntt_basis* basis, uint32_t* src_first, uint32_t* src_count, uint32_t* dst_first, uint32_t* dst_count, int* launches_ntt_form);
AGX_API int agx_ntt_basis_extend(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t batch, int out_form, void* stream);
/* A basis with a PLAINTEXT MODULUS t for its ModDown (BGV): agx_ntt_basis_create's rules in its status order, then t == 0: AGX_ERR_BAD_ARGUMENT, and t = 0
 * modulo a source modulus (t has no inverse there): AGX_ERR_BAD_MODULUS; the out-pointer stays NULL.  Any other 64-bit t is taken -- even, composite, above
 * every modulus -- and reduced per modulus on the host.  t is a property of the basis' ModDown only (agx_ntt_basis_mod_down, _mod_down_mode below):
 * agx_ntt_basis_extend on such a basis writes exactly the words it writes on the ordinary one.  t = 1 gives a basis whose every call equals the ordinary
 * basis' call word for word; agx_ntt_basis_create is this call with t = 1. */
AGX_API int agx_ntt_basis_create_plain(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count,
                                       uint64_t t);

/* ModDown of a hybrid key switch on NTT-form frames: the division of a polynomial known modulo the targets AND the sources of a basis by D = prod q_i
 * over the sources (the special primes), in one call.  Inputs, both in NTT form exactly as agx_ntt_forward / agx_ntt_forward_lazy of the plan write
 * them (bit-reversed order, values in [0,q) or lazy): d_xq dense [T][batch][n], slab j under plan prime dst_first + j; d_xp dense [S][batch][n], slab i
 * under plan prime src_first + i.  Per coefficient of the underlying polynomials (a_j, p_i the coefficient forms of the slabs), with D_i = D / q_i:
 *   y_i = p_i (D_i^-1 mod q_i) mod q_i in [0, q_i),    V = sum_i y_i D_i (an integer, V = X_P + u D, 0 <= u < S),    out_j = (a_j - V) (D^-1 mod q_j) mod q_j,
 * and d_out, dense [T][batch][n], holds NTT_j(out_j), fully reduced: d_out_j = (xq_j - NTT_j(V mod q_j)) D^-1 mod q_j word for word.  This is the
 * APPROXIMATE ModDown of every hybrid key switch, floor(X / D) - u with the u of agx_ntt_basis_extend: a deterministic integer formula, exact against
 * big-integer arithmetic.  With S = 1 it is agx_ntt_rescale(..., AGX_RESCALE_FLOOR) word for word.  This call is the FLOOR mode; agx_ntt_basis_mod_down_mode
 * below has the rounding mode, and on a basis made by agx_ntt_basis_create_plain both keep the value modulo its t.
 * d_scratch: S*batch*n words of device memory; it receives the scaled coefficient form y_i of the source slabs, its contents afterwards are
 * unspecified.  It may be exactly d_xp: the caller thereby GIVES THOSE SLABS UP, as agx_ntt_rescale allows for its last slab; otherwise it is disjoint
 * from d_xp and d_xp is left unchanged.  Aliasing: d_out == d_xq is allowed (in place); any other contact between d_out and d_xq, d_out touching d_xp or
 * the scratch, the scratch touching d_xq, or the scratch partially overlapping d_xp: AGX_ERR_BAD_ARGUMENT, nothing written.  Pointers need 8-byte
 * alignment only.  Ranges that meet end to end do not touch.
 * Status order: a NULL pointer: AGX_ERR_NULL_POINTER; alignment, a layout extent past 2^60 words, on the two-launch route T ceil(batch / frames per
 * workgroup) workgroups past 2^31 - 1, overlap: AGX_ERR_BAD_ARGUMENT; a target modulus equal to a source modulus -- D is not invertible there; any basis
 * whose ranges overlap -- AGX_ERR_BAD_MODULUS (decided at the call: agx_ntt_basis_create accepts such bases for agx_ntt_basis_extend); a plan without
 * inverse tables: AGX_ERR_NO_INVERSE; batch == 0: AGX_OK, nothing launched.  Asynchronous on `stream`, allocates and synchronises nothing
 * (capturable into a hipGraph); agx_ntt_plan_set_variant between calls stays legal.
 * TWO launches for n = 1024 ... 32768 whenever some modulus is 2^31 or larger: the plan's inverse of the S source slabs into the scratch with
 * n^-1 D_i^-1 in the place of n^-1 (the inverse is linear, so it writes y_i itself, at no cost: the constants live in the basis, plan creation is
 * unchanged and no second plan is needed); then, one target prime's frame on chip, the sum over the sources, the forward transform and the difference
 * with xq_j as it streams in (T workgroups per frame; S Shoup products per output word) -- at every S up to 16 (timed at S = 1, 2 and 4:
 * profiles/r09_mod_down.md; tested word for word at every S = 1 ... 16, on this route and on the four-launch one: tests/test_gpu_source_counts.py).
 * Otherwise -- n <= 512, plans whose moduli are all below 2^31, plans forced onto AGX_VARIANT_LDS_RADIX2 -- the inverse of xq into out, the scaled
 * inverse of xp into the scratch, one coefficient-domain pass over out and the plan's forward of out in place: four launches (seven at n = 32768 under
 * AGX_VARIANT_LDS_RADIX2, whose transforms take two each); no memory beyond the scratch, and in place works as in agx_ntt_rescale.
 * agx_ntt_basis_mod_down_info: the kernel launches a call takes under the plan's CURRENT variant; `launches` may be NULL.
 * Groups: no group form, as for agx_ntt_basis_extend: one basis per shard, called on that shard's device and stream. */
AGX_API int agx_ntt_basis_mod_down(const agx_ntt_basis* basis, const uint64_t* d_xq, const uint64_t* d_xp, uint64_t* d_out, uint64_t* d_scratch,
                                   uint64_t batch, void* stream);
AGX_API int agx_ntt_basis_mod_down_info(const agx_ntt_basis* basis, int* launches);
/* ModDown with a rounding mode and the basis' plaintext modulus t (1 on a basis of agx_ntt_basis_create).  Per coefficient, with a_j, p_i, D and D_i as
 * above, h = floor(D / 2) under AGX_RESCALE_ROUND and h = 0 under AGX_RESCALE_FLOOR:
 *   y_i   = ((p_i t^-1 mod q_i) + (h mod q_i)) D_i^-1 mod q_i        in [0, q_i)
 *   V     = sum_i y_i D_i                                             (an integer, 0 <= V < S D)
 *   out_j = (a_j - (t mod q_j) ((V - h) mod q_j)) D^-1 mod q_j        fully reduced
 * delta = t (V - h) satisfies delta = X (mod D) and delta = 0 (mod t), so (X - delta) / D is an exact integer that equals X D^-1 modulo t: the BGV modulus
 * switch and key-switch ModDown (the outputs carry the factor D^-1 mod t, which the caller tracks).  With t = 1: FLOOR is agx_ntt_basis_mod_down word for
 * word, ROUND is floor((X + h) / D) - u with the same 0 <= u < S; with S = 1 and t = 1 it is agx_ntt_rescale in the same mode word for word (u = 0) -- at
 * ANY level of one plan: sources {L - 1}, targets [0, L - 1).  A deterministic integer formula, exact against big-integer arithmetic.
 * Operands, scratch rule, aliasing, status order, launch counts (agx_ntt_basis_mod_down_info serves both modes) and graph capturability are
 * agx_ntt_basis_mod_down's, with one rule right behind the NULL rule, as in agx_ntt_rescale: a mode other than the two: AGX_ERR_BAD_ARGUMENT, nothing
 * written.  agx_ntt_basis_mod_down on any basis is this call with AGX_RESCALE_FLOOR, and FLOOR launches the kernels that call always launched: t lives in
 * the basis' constants alone (t^-1 in the scaled inverse's, a matrix t D_i mod q_j of ModDown's own) and costs no instruction.  ROUND launches kernels of
 * its own with two more steps per word, both with wave-uniform constants: c_i = h D_i^-1 mod q_i joins y_i modulo q_i as the sources stream in, and
 * t h mod q_j leaves the accumulators before the forward passes: S + 1 add-and-conditional-subtract pairs per word beside S Shoup products and a
 * transform.  Measured (profiles/r14_mod_down_modes.md; S = 1, 2, 4 -> T = 4, 60-bit, n = 4096 with 4,096 frames per prime and n = 16384 with 1,024): ROUND takes
 * 1.03 ... 1.05 of FLOOR's time, outside FLOOR's run-to-run spread in five of the six rows (469 against 449 us at S = 1, n = 4096; 1037 against 1005 us at S = 4,
 * n = 16384); a basis with t = 65537 takes 0.995 ... 1.007 of the ordinary basis' time, inside the spread; FLOOR is level with what agx_ntt_basis_mod_down took
 * before this call existed. */
AGX_API int agx_ntt_basis_mod_down_mode(const agx_ntt_basis* basis, const uint64_t* d_xq, const uint64_t* d_xp, uint64_t* d_out, uint64_t* d_scratch,
                                        uint64_t batch, int mode, void* stream);

/* The two EXACT base conversions of a BFV multiplication (BEHZ: Bajard, Eynard, Hasan, Zucca, SAC 2016), on a basis with an AUXILIARY PRIME m: one more prime
 * of the plan, outside both ranges of the basis.  agx_ntt_basis_extend leaves V = X + u D with 0 <= u < S; these two remove u D by integer formulas through m
 * -- no floating point, no rounded quotient estimate; exact against big-integer arithmetic like every RNS call here.  With D, D_i as above, x' = x mod q and
 * centre(a) = a for a in [0, (m - 1) / 2], a - m for a above (m is odd, so centre(-a mod m) = -centre(a)):
 * agx_ntt_basis_extend_exact, the Shenoy-Kumaresan conversion.  Inputs in coefficient form: x_i under the S sources, values in [0, 4 q_i); r under m, values
 * in [0, 4m).
 *   y_i = x_i' D_i^-1 mod q_i in [0, q_i),    V = sum_i y_i D_i,    alpha = centre(((V - r') D^-1) mod m),    out_j = (V - alpha D) mod q_j, fully reduced.
 * Property: let X' be an integer with X' = x_i (mod q_i) for every source and r = X' (mod m); write X' = X + k D with X in [0, D), and V = X + u D.  Whenever
 * |u - k| <= (m - 1) / 2, out_j = X' mod q_j exactly: it is exact for every X' with |X'| < ((m - 1) / 2 - S) D, negative ones included.  The formula, not the
 * property, is the contract; it is defined for every input.
 * agx_ntt_basis_extend_mont, BEHZ's FastBConv_m~ followed by SmMRq_m~ (the small Montgomery reduction).  Inputs: x_i under the sources, coefficient form,
 * values in [0, 4 q_i).
 *   y_i = x_i' (m D_i^-1) mod q_i,    V = sum_i y_i D_i,    alpha = centre((-V D^-1) mod m),    out_j = (V + alpha D) m^-1 mod q_j, fully reduced.
 * Property: W = (V + alpha D) / m is an exact integer and W = X (mod D); when m > 2S, W is X - D or X, with -D/2 < W < D/2 + S D / m: the u D of the approximate
 * conversion shrinks to at most one D, on the centred side, which keeps the noise of the tensor product small.  out_j = W mod q_j.
 *   create_aux : agx_ntt_basis_create's rules in its status order, then aux_prime >= P or inside the source or the target range: AGX_ERR_BAD_ARGUMENT; m equal
 *                to a source or target modulus: AGX_ERR_BAD_MODULUS.  On any failure the out-pointer is cleared.  The basis has t = 1, and
 *                agx_ntt_basis_extend, _mod_down and _mod_down_mode behave on it word for word as on the basis of agx_ntt_basis_create with the same ranges.
 *   aux_info   : has_aux (0 on an ordinary basis), the auxiliary prime's index, and launches_ntt_form = 1 + the launches of the plan's forward under its
 *                CURRENT variant.  Any out-pointer may be NULL.
 *   the calls  : d_x dense [S][batch][n], d_xaux dense [1][batch][n], d_out dense [T][batch][n]; out_form as in agx_ntt_basis_extend.  Pointers need 8-byte
 *                alignment only.  OUT OF PLACE ONLY: d_out touches neither d_x nor d_xaux; d_x and d_xaux may overlap freely (in a BFV multiplication d_xaux
 *                is the slab that follows d_x's); ranges that meet end to end do not touch.  Status order: agx_ntt_basis_extend's, with one rule right behind
 *                the NULL rule: a basis without an auxiliary prime: AGX_ERR_BAD_ARGUMENT, nothing written.  batch == 0: AGX_OK, nothing launched.
 *                Asynchronous on `stream`, allocates and synchronises nothing (capturable into a hipGraph).  Any plan serves, forward-only plans included.
 * AGX_FORM_COEFF is ONE launch on every plan, the shape of agx_ntt_basis_extend's: one thread per coefficient reads its S source words (S + 1: exact), forms
 * V mod m through one more constant row {D_i mod m}, alpha once (one Shoup product by D^-1 mod m and the centring), walks the T targets and finishes each with
 * one Shoup product |alpha| (D mod q_j), added or subtracted by alpha's sign: 8 (S + 1 + T) bytes per coefficient (exact), 8 (S + T) (mont).  m is folded
 * into the D_i^-1 constants and m^-1 into the matrix and D mod q_j: the Montgomery form costs no instruction beyond the exact form, the two are one body
 * with two constant sets (csrc/bfv_conv_arith.hpp has the per-word steps and their range arguments, for any odd modulus below 2^62).  AGX_FORM_NTT is that
 * launch followed by the plan's forward on the target slabs in place; there is no fused one-launch form.  Measured (profiles/r15_bfv_conversions.md; coefficient form, S = 2, 4 -> T = 3, 5, 60-bit, n = 4096 with 4,096
 * frames per prime and n = 16384 with 1,024): exact takes 1.28 ... 1.44 and mont 1.21 ... 1.38 of the time of agx_ntt_basis_extend of the same S into T + 1 targets, outside its
 * run-to-run spread in every row (217 against 153 us at S = 2, T = 3; 464 against 351 us at S = 4, T = 5), and 1.49 ... 1.93 / 1.65 ... 2.01 of a device copy of their model bytes:
 * the kernel is bound by its S + 1 + T additional Shoup products, not by its traffic.  mont's median is 0.94 ... 0.96 of exact's; their spreads overlap in half of the rows.
 * INTEGRATION.md, "BFV multiplication (BEHZ)", has a whole multiplication on these calls.  Groups: no group form, as for agx_ntt_basis_extend. */
AGX_API int agx_ntt_basis_create_aux(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t src_first, uint32_t src_count, uint32_t dst_first, uint32_t dst_count,
                                     uint32_t aux_prime);
AGX_API int agx_ntt_basis_aux_info(const agx_ntt_basis* basis, int* has_aux, uint32_t* aux_prime, int* launches_ntt_form);
AGX_API int agx_ntt_basis_extend_exact(const agx_ntt_basis* basis, const uint64_t* d_x, const uint64_t* d_xaux, uint64_t* d_out, uint64_t batch, int out_form,
                                       void* stream);
AGX_API int agx_ntt_basis_extend_mont(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t batch, int out_form, void* stream);
/* BFV's divide-and-return in one pass: steps 4 to 7 of a BEHZ multiplication ("BFV multiplication (BEHZ)") -- times t, the fast floor of
 * t X / Q on Bsk, and the Shenoy-Kumaresan return to Q -- on one component of the tensor product.  Q = the plan primes [q_first, q_first + L) with product
 * D, Q_i = D / q_i; B = [b_first, b_first + K) with product B, B_j = B / b_j; m = the plan prime aux_prime; Bsk = B u {m}; x' = x mod its modulus; centre as
 * for agx_ntt_basis_extend_exact.  Per coefficient, with a_. the coefficient forms of the slabs of d_x:
 *   y_i   = (t a_i') Q_i^-1 mod q_i  in [0, q_i),        V = sum_i y_i Q_i                     (i in Q)
 *   f_j   = (t a_j' - V) D^-1 mod b_j                                                          (j in B and j = m): floor(t X / D) - u on Bsk
 *   z_j   = f_j B_j^-1 mod b_j       in [0, b_j),        W = sum_j z_j B_j                     (j in B)
 *   alpha = centre((W - f_m) B^-1 mod m),                out_i = (W - alpha B) mod q_i         (i in Q)
 *   d_out = NTT_i(out_i)
 * which is, word for word, agx_ntt_mul_add_galois by a frame of t's, agx_ntt_basis_mod_down on the basis (sources Q, targets Bsk), the inverse on Bsk and
 * agx_ntt_basis_extend_exact(..., AGX_FORM_NTT): six launches, 2L + 2K + 2 frame transforms and a multiply pass, of which the forward and the inverse on
 * Bsk undo each other.  Every formula is an exact integer formula, so this call runs the chain in the coefficient domain: 2L + K + 1 frame transforms,
 * no pass for t, no frame of t's, no second plan.  The return is exact under agx_ntt_basis_extend_exact's bound.
 *   create_quotient : the basis agx_ntt_basis_create_aux(plan, b_first, b_count, q_first, q_count, aux_prime) makes -- sources B, targets Q, auxiliary prime
 *                     m: every call it had (extend, extend_exact, extend_mont, mod_down, mod_down_mode, info, aux_info) behaves on it word for word as on
 *                     that basis -- with the constants of the quotient.  Rules: agx_ntt_basis_create_aux's in its order, with q_count > 16 beside
 *                     b_count > 16; then ranges that overlap: AGX_ERR_BAD_ARGUMENT; two equal moduli among Q, B and m: AGX_ERR_BAD_MODULUS; t == 0:
 *                     AGX_ERR_BAD_ARGUMENT.  Any other 64-bit t is taken and reduced per modulus on the host (t is only multiplied: it needs no
 *                     inverse anywhere).  On any failure the out-pointer is cleared.
 *   quotient_info   : has_quotient (0 on every other basis, where t reads 0), t, and the kernel launches of one call under the plan's CURRENT variant:
 *                     2 x the plan's inverse + 1 + the plan's forward where m is the plan prime right behind B (aux_prime = b_first + b_count: Bsk is one
 *                     range, the layout of the listing), and one inverse more where it is not.  Any out-pointer may be NULL.
 *   quotient        : d_x dense [L + K + 1][batch][n] in NTT form as agx_ntt_forward / _forward_lazy of the plan write it (reduced or lazy), the slabs of Q,
 *                     then of B, then of m: one component of the tensor product on Q u Bsk.  d_out dense [L][batch][n], NTT form under Q, fully reduced.
 *                     d_scratch: (L + K + 1) batch n words; it may be exactly d_x, which is then given up (as agx_ntt_rescale and agx_ntt_basis_mod_down
 *                     allow), otherwise it touches d_x nowhere and d_x is left unchanged; d_out touches neither; ranges that meet end to end do not touch.
 *                     Status order: NULL: AGX_ERR_NULL_POINTER; a basis without the quotient's constants: AGX_ERR_BAD_ARGUMENT; the plan's device not
 *                     current: AGX_ERR_BAD_ARGUMENT; 8-byte alignment, the batch grid limit, an extent past 2^60 words, the overlap rules:
 *                     AGX_ERR_BAD_ARGUMENT, nothing written; a plan without inverse tables: AGX_ERR_NO_INVERSE; batch == 0: AGX_OK, nothing launched.
 *                     Asynchronous; allocates and synchronises nothing (capturable into a hipGraph); agx_ntt_plan_set_variant between calls stays legal.
 * Route, one for every plan: the plan's inverse on the view of Q into the scratch with n^-1 t Q_i^-1 in the place of n^-1, so it writes the y_i (the
 * mechanism of agx_ntt_basis_mod_down); the plan's inverse on the view of Bsk with n^-1 t D^-1 B_j^-1 (m: n^-1 t D^-1); ONE streaming kernel, one thread
 * per coefficient, no LDS: z_j = s_j - sum_i y_i (q_i^-1 B_j^-1 mod b_j) since D^-1 Q_i = q_i^-1, f_m by the row q_i^-1 mod m, W mod m, alpha by one Shoup
 * product and the centring, out_i = sum_j z_j (B_j mod q_i) -+ |alpha| (B mod q_i) -- 8 (2L + K + 1) bytes per coefficient, K + 2 words live; then the plan's
 * forward on the view of Q, in place in d_out.
 * Measured on an MI355X (profiles/r16_bfv_quotient.md, tools/run_op.py --op quotient; 60-bit primes, L = K = 2 and 4, n = 4096 with 4,096 frames per prime and
 * n = 16384 with 1,024, the scratch the operand): 0.62 ... 0.66 of the time of the six-call composition on the same buffer, outside the spreads in every row
 * (L = K = 2 at n = 4096: 753 us against 1216 us; L = K = 4: 1556 against 2371), and 4.1 ... 5.0 of the time of a device copy of its model bytes,
 * 8 (2L + K + 1) per coefficient: the call is three transform launches and the kernel, and moves three times those bytes.
 * Groups: no group form, as for agx_ntt_basis_extend. */
AGX_API int agx_ntt_basis_create_quotient(agx_ntt_basis** basis, const agx_ntt_plan* plan, uint32_t b_first, uint32_t b_count, uint32_t q_first, uint32_t q_count,
                                          uint32_t aux_prime, uint64_t t);
AGX_API int agx_ntt_basis_quotient_info(const agx_ntt_basis* basis, int* has_quotient, uint64_t* t, int* launches);
AGX_API int agx_ntt_basis_quotient(const agx_ntt_basis* basis, const uint64_t* d_x, uint64_t* d_out, uint64_t* d_scratch, uint64_t batch, void* stream);

/* The inner product of NTT-form frames: c_o = sum_t a_t o bhat_{t,o} mod q for o < outputs, one launch -- the centre of a hybrid key switch (the sum over
 * the decomposition digits of digit times key), and any other multiply-accumulate against operands kept in NTT form.  P = the plan's primes:
 *   d_a    dense [terms][P][batch][n]
 *   d_bhat dense [terms][outputs][P][bhat_batch][n], bhat_batch == batch (frame by frame) or bhat_batch == 1 (one key frame per prime, used for every frame
 *          of the batch: the key is stored once, not once per frame)
 *   d_c    dense [outputs][P][batch][n]
 * Every input word may lie in [0, 4 q_p), as agx_ntt_forward_lazy leaves them and agx_ntt_pointwise accepts them; the output is fully reduced.  Per word
 *   c_o[p][b][i] = (sum_t (a_t[p][b][i] mod q_p) (bhat_{t,o}[p][b or 0][i] mod q_p)) mod q_p,
 * exact against big-integer arithmetic.  Positions are not interpreted: any order that both operands share.  terms = outputs = 1 with bhat_batch == batch is
 * agx_ntt_pointwise word for word.  terms <= AGX_INNER_MAX_TERMS = 16 is part of the contract: reduced operands give products below 2^124, sixteen of them
 * stay below 2^128, so the sum is kept in 128 bits and reduced ONCE (the argument of AGX_BASIS_MAX_SRC; csrc/inner_reduce.hpp has the reduction's).
 * Every plan serves, whatever its variant, size and moduli; no inverse tables are needed and plan creation is unchanged.
 * Status order: a NULL pointer: AGX_ERR_NULL_POINTER; terms 0 or above 16, outputs 0 or above AGX_INNER_MAX_OUTPUTS = 2, bhat_batch neither batch nor 1; a
 * pointer not 8-byte aligned; a batch past the grid limit or an operand's extent past 2^60 words; d_c's range touching d_a's or d_bhat's anywhere, equal
 * pointers included (OUT OF PLACE ONLY, as agx_ntt_automorphism); the plan's device not current: AGX_ERR_BAD_ARGUMENT, nothing written; batch == 0: AGX_OK,
 * nothing launched.  Asynchronous on `stream`, allocates and synchronises nothing, touches no plan state (capturable into a hipGraph).
 * ONE launch: a grid-stride streaming kernel, no LDS, no barrier, no table; 16-byte accesses when all three bases are 16-byte aligned, 8-byte ones otherwise.
 * It moves 8 (terms + outputs) bytes per word of a frame plus the key (8 terms outputs more per word with bhat_batch == batch; with bhat_batch == 1 the key's
 * own size once, its repeats served by L2), where terms x outputs agx_ntt_pointwise calls and caller-side adds move about 24 per term and output.  Measured
 * (profiles/r10_keyswitch.md; four 60-bit primes, two outputs, terms 2 ... 4, n = 4096 with 4,096 frames per prime and n = 16384 with 1,024): 0.89 ... 1.16 of the
 * time of a device copy of the model's bytes; 0.17 ... 0.22 (bhat_batch == 1) and 0.36 ... 0.41 (bhat_batch == batch) of the pointwise-and-add form's. */
#define AGX_INNER_MAX_TERMS 16
#define AGX_INNER_MAX_OUTPUTS 2
AGX_API int agx_ntt_inner_product(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_bhat, uint64_t* d_c, uint64_t batch, uint64_t bhat_batch,
                                  uint32_t terms, uint32_t outputs, void* stream);

/* The inner product with `a` read through a Galois automorphism: operands, layouts, ranges, limits and status order are agx_ntt_inner_product's.  Per word,
 * with pi_g(i) = brev((g brev(i) + (g - 1) / 2) mod n), the permutation agx_ntt_automorphism applies to an NTT-form frame,
 *   c_o[p][b][i] = (sum_t (a_t[p][b][pi_g(i)] mod q_p) (bhat_{t,o}[p][b or 0][i] mod q_p)) mod q_p.
 * Only `a` is read through pi_g; the key and c sit at natural positions.  Word for word this is agx_ntt_automorphism(AGX_FORM_NTT, g) on every frame of `a`
 * followed by agx_ntt_inner_product, without the permuted copy of `a` or the scratch it would need; galois_elt = 1 is agx_ntt_inner_product itself (and runs
 * its kernel).  One rule is added, checked after the overlap rule and before the device's: galois_elt even, 0 or >= 2n: AGX_ERR_BAD_ARGUMENT, nothing written.
 * Out of place, asynchronous, allocates nothing, touches no plan state, capturable into a hipGraph; ONE launch on every plan: the same streaming kernel with
 * pi_g formed once per work item, no LDS, no barrier, no table; 16-byte accesses when all three bases are 16-byte aligned (an output pair reads one input
 * pair, its halves swapped or not), 8-byte ones otherwise.  A wave reads the same aligned segments of `a` as the plain kernel, in another lane order.
 * Measured (profiles/r11_hoisted_rotations.md; six 60-bit primes, key switch shapes (4, 4, 2, 2) and (3, 4, 2, 2): two terms, two outputs, broadcast key over 6 and
 * 5 primes, g = 5, n = 4096 with 4,096 frames per prime and n = 16384 with 1,024): 1.07 of the time of agx_ntt_inner_product in all four rows (737 against 686 us at n = 4096
 * over 6 primes) -- SLOWER than the plain kernel by 7 %, the min ... max spreads do not overlap -- and 0.60 of agx_ntt_automorphism into a permuted copy followed by
 * agx_ntt_inner_product (1227 us), which also needs terms P batch n words for that copy. */
AGX_API int agx_ntt_inner_product_galois(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_bhat, uint64_t* d_c, uint64_t batch,
                                         uint64_t bhat_batch, uint32_t terms, uint32_t outputs, uint32_t galois_elt, void* stream);

/* Ring arithmetic on NTT-form frames over a RANGE of the plan's primes: add, subtract, negate, add through a Galois automorphism, and the tensor product of
 * two ciphertexts.  With them a homomorphic multiplication (tensor, agx_ntt_keyswitch_apply on c_2, two adds, agx_ntt_rescale) and a hoisted rotation
 * (decompose, apply_decomposed, add_galois) run on library calls alone, at any level of one plan.
 * All five serve the plan primes [prime_first, prime_first + prime_count); every operand set is dense [prime_count][batch][n], slab i under plan prime
 * prime_first + i, as agx_ntt_basis_create names its ranges; a ciphertext at level q_count passes (0, q_count).  For agx_ntt_tensor a and b are
 * [2][prime_count][batch][n] and c is [3][prime_count][batch][n].  Every input word may lie in [0, 4 q_p), as agx_ntt_forward_lazy leaves them; every output
 * is fully reduced and exact against big-integer arithmetic on the residues.  Positions are not interpreted -- any order that all operands share -- except by
 * add_galois.  Per word, with x' = x mod q_p:
 *   add        c = (a' + b') mod q_p                 sub     c = (a' - b') mod q_p                 negate  c = (-a') mod q_p, -0 = 0
 *   add_galois c[p][f][i] = (a[p][f][i]' + b[p][f][pi_g(i)]') mod q_p, pi_g(i) = brev((g brev(i) + (g - 1) / 2) mod n): a + agx_ntt_automorphism(AGX_FORM_NTT, g) of b,
 *              without the permuted copy of b; galois_elt = 1 is agx_ntt_add word for word and runs its kernel
 *   tensor     c_0 = a_0 o b_0,   c_1 = a_0 o b_1 + a_1 o b_0,   c_2 = a_1 o b_1, all mod q_p; the cross term is summed in 128 bits and reduced once
 * Every plan serves, whatever its variant, size and moduli; no inverse tables are needed and plan creation is unchanged.
 * Aliasing.  add, sub: d_c may be exactly d_a, exactly d_b, or both; d_a and d_b may overlap in any way (both are only read).  negate: d_c may be exactly d_a.
 * add_galois: d_c may be exactly d_a (the in-place out_0 += sigma_g(c0)); d_c may not touch d_b anywhere, since b is gathered across the frame -- with
 * galois_elt = 1, as for add, it may be d_b.  tensor: OUT OF PLACE ONLY, d_c's range touches neither d_a's nor d_b's; d_a == d_b squares, and they may overlap
 * freely.  Every other contact -- a partial overlap of c with an operand it may equal, any contact with one it may not touch -- is AGX_ERR_BAD_ARGUMENT.
 * Ranges that meet end to end do not touch.
 * Status order of the five, agx_ntt_inner_product's: a NULL plan or pointer: AGX_ERR_NULL_POINTER; prime_count == 0 or a range past P; a pointer not 8-byte
 * aligned; a batch past the grid limit; an operand's extent past 2^60 words; the aliasing rules above; add_galois only: galois_elt even, 0 or >= 2n; the
 * plan's device not current: AGX_ERR_BAD_ARGUMENT, nothing written; batch == 0: AGX_OK, nothing launched.
 * Asynchronous on `stream`; they allocate nothing, synchronise nothing and touch no plan state (capturable into a hipGraph).  ONE launch each: a grid-stride
 * streaming kernel, no LDS, no barrier, no table; 16-byte accesses when ALL bases of the call are 16-byte aligned, 8-byte ones otherwise.  They move 24 bytes
 * per word (add, sub, add_galois), 16 (negate) and 56 per word of a frame (tensor: four words read, three written), where four agx_ntt_pointwise launches
 * move 96 and leave the cross term's add to the caller, and agx_ntt_automorphism into a copy followed by an add moves 40 and needs the copy's memory.
 * Measured (profiles/r12_ring_ops.md; six 60-bit primes, range (0, 4), n = 4096 with 4,096 frames per prime and n = 16384 with 1,024, 16-byte bases, g = 5), beside a
 * device copy of the model's bytes in the same process: add 280 / 281 us (0.94 / 0.89 of the copy), sub 281 / 283 (0.94 / 0.85), negate 180 / 181 (0.90 / 0.94), add_galois
 * 284 / 293 (0.91 / 0.95; 1 % and 4 % above the plain add, the spreads apart) and 0.40 / 0.41 of agx_ntt_automorphism into a copy plus an add; tensor 699 / 745 us: 0.94 of the
 * copy at n = 4096 and 1.00 at n = 16384, where its spread and the copy's overlap -- level with the copy there, not ahead -- and 0.65 / 0.68 of four agx_ntt_pointwise launches.
 * Groups: no group form, as for the other RNS calls: each shard calls them on its own plan. */
AGX_API int agx_ntt_add(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, uint32_t prime_first,
                        uint32_t prime_count, void* stream);
AGX_API int agx_ntt_sub(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, uint32_t prime_first,
                        uint32_t prime_count, void* stream);
AGX_API int agx_ntt_negate(const agx_ntt_plan* plan, const uint64_t* d_a, uint64_t* d_c, uint64_t batch, uint32_t prime_first, uint32_t prime_count, void* stream);
AGX_API int agx_ntt_add_galois(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, uint32_t prime_first,
                               uint32_t prime_count, uint32_t galois_elt, void* stream);
AGX_API int agx_ntt_tensor(const agx_ntt_plan* plan, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_c, uint64_t batch, uint32_t prime_first,
                           uint32_t prime_count, void* stream);

/* Multiply-accumulate on a range of the plan's primes with a broadcast operand, read through a Galois automorphism: the plaintext x ciphertext product at a
 * level, and the way the sigma_g(c0) terms and an unrotated diagonal join a linear transform's sum (agx_ntt_keyswitch_accumulate_decomposed below).  The range
 * and the operands are the ring calls' above: d_b and d_c are [prime_count][batch][n]; d_w is [prime_count][w_batch][n] with w_batch = batch or 1 (1: one
 * frame per prime for every frame of the batch).  Per word, with x' = x mod q_p and pi_g as for add_galois:
 *   c[p][f][i] = ((accumulate ? c[p][f][i]' : 0) + w[p][f or 0][i]' b[p][f][pi_g(i)]') mod q_p
 * Inputs (the old words of c included) may be lazy, below 4 q_p; the output is fully reduced and exact: w' b' + c' < 2^124 + 2^62 is kept in 128 bits and
 * reduced once.  accumulate is 0 or 1.  With galois_elt = 1 and accumulate = 0 this is the ranged plaintext product; with w_batch == batch over the whole
 * plan it equals agx_ntt_pointwise word for word; with w all ones it is agx_ntt_automorphism(AGX_FORM_NTT, g) reduced (accumulate = 0) or agx_ntt_add_galois
 * (accumulate = 1).
 * Aliasing.  d_c touches d_w nowhere.  d_c touches d_b nowhere, except that with galois_elt = 1 it may be exactly d_b (the in-place plaintext multiply).
 * d_w and d_b may overlap freely (both are only read).  Ranges that meet end to end do not touch.
 * Status order, agx_ntt_add_galois's: a NULL plan or pointer: AGX_ERR_NULL_POINTER; prime_count == 0 or a range past P, w_batch neither batch nor 1, accumulate
 * neither 0 nor 1; a pointer not 8-byte aligned; a batch past the grid limit; an operand's extent past 2^60 words; the aliasing rules above; galois_elt even, 0
 * or >= 2n; the plan's device not current: AGX_ERR_BAD_ARGUMENT, nothing written; batch == 0: AGX_OK, nothing launched.
 * Asynchronous on `stream`; allocates nothing, synchronises nothing, touches no plan state (capturable into a hipGraph).  ONE launch on every plan: a
 * grid-stride streaming kernel, no LDS, no barrier, no table; 16-byte accesses when all three bases are 16-byte aligned; galois_elt = 1 takes an un-gathered
 * kernel.  It moves 16 bytes per word of a frame, 8 more with accumulate = 1 and 8 more with w_batch == batch.
 * Measured: not measured yet on its own; within a linear transform, see agx_ntt_keyswitch_accumulate_decomposed (profiles/r13_double_hoisting.md).
 * Groups: no group form, as for the other RNS calls. */
AGX_API int agx_ntt_mul_add_galois(const agx_ntt_plan* plan, const uint64_t* d_w, uint64_t w_batch, const uint64_t* d_b, uint64_t* d_c, uint64_t batch,
                                   uint32_t prime_first, uint32_t prime_count, uint32_t galois_elt, int accumulate, void* stream);

/* The RNS hybrid key switch of one ciphertext component in one call: NTT form in, NTT form out, at any level.
 * Primes.  Q, the ciphertext's current level, is the plan's primes [0, q_count).  The special primes are [p_first, p_first + p_count), p_first >= q_count:
 * they need not follow Q directly, which is what a level below the top looks like.  The ACTIVE primes are Q followed by the special primes, A = q_count +
 * p_count of them.  Digit d is the primes [d alpha, min((d + 1) alpha, q_count)) -- the last digit may be short -- and digits = ceil(q_count / alpha).
 *   d_chat    [q_count][batch][n]    NTT form of this plan, values in [0,q) or lazy; left unchanged
 *   d_keyhat  [digits][2][A][n]      NTT form under the active primes in that order, reduced or lazy; shared by every frame of the batch
 *   d_out     [2][q_count][batch][n] NTT form, fully reduced
 *   d_scratch the words agx_ntt_keyswitch_scratch_words reports ((q_count + (digits + 2) A) batch n); contents unspecified afterwards
 * Definition, per coefficient, from the formulas above:
 *   1. c_j = INTT_j(chat_j) in [0, q_j) for j in Q.
 *   2. For digit d with sources S_d, D_d = prod q_i and D_{d,i} = D_d / q_i:  y_i = c_i D_{d,i}^-1 mod q_i,  V_d = sum_i y_i D_{d,i},  e_{d,j} = V_d mod q_j for
 *      every active j: agx_ntt_basis_extend's conversion (so e_{d,j} = c_j for j in S_d).
 *   3. acc_{o,j} = sum_d NTT_j(e_{d,j}) o key_{d,o,j} mod q_j for o = 0, 1 and every active j: one agx_ntt_inner_product over the active primes.
 *   4. out_{o,j} = agx_ntt_basis_mod_down's result with targets Q and sources the special primes on acc_o: (acc_{o,j} - NTT_j(V mod q_j)) D_P^-1 mod q_j.
 * A deterministic integer formula: every output word is exact against big-integer arithmetic.
 * A handle owns the bases -- one ModUp basis per digit when p_first == q_count, two per digit (targets Q, targets P) when the special primes lie apart, one
 * ModDown basis -- and a pointer to the plan, none of its tables: the plan must outlive it, agx_ntt_plan_set_variant between calls stays legal, and the
 * plan's device must be current at creation and at every apply.  Step 1 is the plan's inverse on the view of primes [0, q_count): no second plan.  Steps 2
 * and 4 are the public calls themselves, so their route choices (profiles/r08_basis_extend.md, r09_mod_down.md) apply unchanged; ModDown's scratch is the
 * special slabs of acc_o.  Everything is issued on the one stream passed.
 *   create : NULL: AGX_ERR_NULL_POINTER; q_count == 0, p_count == 0, alpha == 0, alpha or p_count above AGX_BASIS_MAX_SRC, digits above
 *            AGX_KEYSWITCH_MAX_DIGITS = 16, p_first < q_count, a range past P: AGX_ERR_BAD_ARGUMENT; two equal moduli among the active primes:
 *            AGX_ERR_BAD_MODULUS.        destroy: NULL is fine.
 *   info   : the shape, digits, and launches = the kernel launches of one apply under the plan's CURRENT variant: the inverse on Q + what agx_ntt_basis_info
 *            reports for every ModUp basis + 1 (the inner product) + 2 x what agx_ntt_basis_mod_down_info reports.  Any out-pointer may be NULL.
 *   scratch_words : NULL: AGX_ERR_NULL_POINTER; a count past 2^60 words: AGX_ERR_BAD_ARGUMENT.
 *   apply  : status order: a NULL pointer: AGX_ERR_NULL_POINTER; a pointer not 8-byte aligned, a batch past the grid limit or with A batch above 2^31 - 1, an
 *            extent past 2^60 words, any two of chat / keyhat / out / scratch touching anywhere, the plan's device not current: AGX_ERR_BAD_ARGUMENT, nothing
 *            written; a plan without inverse tables: AGX_ERR_NO_INVERSE; batch == 0: AGX_OK, nothing launched.  Ranges that meet end to end do not touch.
 *            Asynchronous on `stream`, allocates and synchronises nothing (capturable into a hipGraph).
 * Groups: no group form, as for bases: each shard makes one handle on its own plan. */
#define AGX_KEYSWITCH_MAX_DIGITS 16
typedef struct agx_ntt_keyswitch agx_ntt_keyswitch;
AGX_API int agx_ntt_keyswitch_create(agx_ntt_keyswitch** ks, const agx_ntt_plan* plan, uint32_t q_count, uint32_t p_first, uint32_t p_count, uint32_t alpha);
AGX_API int agx_ntt_keyswitch_destroy(agx_ntt_keyswitch* ks);
AGX_API int agx_ntt_keyswitch_info(const agx_ntt_keyswitch* ks, uint32_t* q_count, uint32_t* p_first, uint32_t* p_count, uint32_t* alpha, uint32_t* digits,
                                   int* launches);
AGX_API int agx_ntt_keyswitch_scratch_words(const agx_ntt_keyswitch* ks, uint64_t batch, uint64_t* words);
AGX_API int agx_ntt_keyswitch_apply(const agx_ntt_keyswitch* ks, const uint64_t* d_chat, const uint64_t* d_keyhat, uint64_t* d_out, uint64_t* d_scratch,
                                    uint64_t batch, void* stream);
/* agx_ntt_keyswitch_create with the ModDown basis made by agx_ntt_basis_create_plain(..., t): the BGV key switch.  The ModUp bases are unchanged.  Every
 * call on the handle then divides by P keeping the value modulo t (step 4 above in the FLOOR mode of agx_ntt_basis_mod_down_mode): apply, apply_decomposed,
 * agx_ntt_keyswitch_mod_down and the double-hoisted route.  Status: agx_ntt_keyswitch_create's rules in its order, then t == 0: AGX_ERR_BAD_ARGUMENT; t = 0
 * modulo a special prime: AGX_ERR_BAD_MODULUS; the out-pointer stays NULL.  t = 1 is agx_ntt_keyswitch_create.  There is no rounding inside the key
 * switch's ModDown. */
AGX_API int agx_ntt_keyswitch_create_plain(agx_ntt_keyswitch** ks, const agx_ntt_plan* plan, uint32_t q_count, uint32_t p_first, uint32_t p_count, uint32_t alpha,
                                           uint64_t t);

/* The key switch in two halves, for rotating ONE ciphertext by several steps (hoisting, Halevi-Shoup): steps 1 and 2 above depend on the ciphertext alone,
 * so they are done once, and every Galois element g pays for steps 3 and 4 only.  Both calls work on an agx_ntt_keyswitch handle as created above.
 *   decompose        : steps 1 and 2.  d_chat [q_count][batch][n] as for apply, left unchanged; d_ext [digits][A][batch][n] receives NTT_j(e_{d,j}), fully
 *                      reduced: exactly the words apply forms in the ext part of its scratch; d_scratch: q_count batch n words (the coefficient form).
 *   apply_decomposed : steps 3 and 4 with ext read through pi_g (agx_ntt_inner_product_galois): acc_{o,j} = sum_d pi_g(ext_{d,j}) o key_{d,o,j}, one launch
 *                      over the active primes with the key broadcast, then the two agx_ntt_basis_mod_down calls of step 4, the special slabs of acc_o their
 *                      scratch.  d_ext is const and unchanged: one decomposition serves any number of Galois elements and keys.  d_keyhat [digits][2][A][n]
 *                      and d_out [2][q_count][batch][n] (fully reduced) as for apply; d_scratch: 2 A batch n words.
 * What it computes.  pi_g(ext_d) is the NTT form of sigma_g(V_d) mod q_j (sigma_g: X -> X^g), consistently over every active j, and sigma_g(V_d) is an integer
 * polynomial with coefficients in (-S D_d, S D_d), S the digit's source count, congruent to sigma_g(c) modulo D_d.  So the call key-switches sigma_g(c) with a
 * key for sigma_g(s) -> s, and every output word is exact against big-integer arithmetic.  For g != 1 the result is NOT word-equal to agx_ntt_automorphism on
 * chat followed by apply: the approximate lift does not commute with negation, and the two results differ by what both approximate conversions already leave
 * to the noise.  For g = 1, decompose followed by apply_decomposed equals apply word for word (apply IS the two halves on the parts of its scratch).  Adding
 * sigma_g(c0) to out_0 is agx_ntt_add_galois(plan, out_0, c0, out_0, batch, 0, q_count, g, stream), in place.
 *   hoisted_words : the sizes in words of d_ext, decompose's scratch and apply_decomposed's scratch: the ext, coeff and acc parts of scratch_words.  A NULL
 *                   handle: AGX_ERR_NULL_POINTER; a count past 2^60 words: AGX_ERR_BAD_ARGUMENT; any out-pointer may be NULL.
 *   hoisted_info  : launches_decompose = the inverse on Q + what agx_ntt_basis_info reports for every ModUp basis; launches_apply_decomposed = 1 + 2 x what
 *                   agx_ntt_basis_mod_down_info reports; their sum is agx_ntt_keyswitch_info's launches.  Under the plan's CURRENT variant; either may be NULL.
 *   Status order of both halves, as apply: a NULL pointer: AGX_ERR_NULL_POINTER; a pointer not 8-byte aligned, a batch past the grid limit or with A batch above
 *   2^31 - 1, an extent past 2^60 words, any two of the call's buffers touching anywhere (ranges that meet end to end do not touch); then, apply_decomposed
 *   only, galois_elt even, 0 or >= 2n; then the plan's device not current: AGX_ERR_BAD_ARGUMENT, nothing written; a plan without inverse tables:
 *   AGX_ERR_NO_INVERSE; batch == 0: AGX_OK, nothing launched.  Asynchronous on `stream`, allocate and synchronise nothing (capturable into a hipGraph).
 * Measured (profiles/r11_hoisted_rotations.md; six 60-bit primes, g = 5 and its powers): at n = 4096, (4, 4, 2, 2), 4,096 frames per prime decompose takes 1434 us and
 * one apply_decomposed 1908 us, together 1.013 of apply's 3299 us (1.010 ... 1.015 over the four rows: the gathered inner product costs 7 % more than the plain one).  Against R x
 * (agx_ntt_automorphism on chat + apply), decompose once + R x apply_decomposed takes 0.97 at R = 1, 0.66 at R = 4 and 0.60 at R = 8 (16.75 against 27.76 ms); over both shapes and
 * n = 4096 / 16384: 0.965 ... 0.976, 0.642 ... 0.659, 0.587 ... 0.606.  apply itself, beside the library before the split in the same session: 3327 against 3333 us, 2746 / 2747,
 * 3840 / 3841, 3128 / 3128 -- the spreads overlap in every row.
 * Groups: no group form, as for bases and key switches: each shard calls the halves on its own handle. */
AGX_API int agx_ntt_keyswitch_hoisted_words(const agx_ntt_keyswitch* ks, uint64_t batch, uint64_t* ext_words, uint64_t* decompose_scratch_words,
                                            uint64_t* apply_scratch_words);
AGX_API int agx_ntt_keyswitch_decompose(const agx_ntt_keyswitch* ks, const uint64_t* d_chat, uint64_t* d_ext, uint64_t* d_scratch, uint64_t batch, void* stream);
AGX_API int agx_ntt_keyswitch_apply_decomposed(const agx_ntt_keyswitch* ks, const uint64_t* d_ext, const uint64_t* d_keyhat, uint64_t* d_out,
                                               uint64_t* d_scratch, uint64_t batch, uint32_t galois_elt, void* stream);
AGX_API int agx_ntt_keyswitch_hoisted_info(const agx_ntt_keyswitch* ks, int* launches_decompose, int* launches_apply_decomposed);

/* apply_decomposed in ITS two halves, for a linear transform out = sum_r w_r o sigma_{g_r}(ct) (matrix-vector products by diagonals, the BSGS inner loop,
 * CoeffToSlot / SlotToCoeff): ModDown is linear, so the sum over the rotations is formed in the extended basis Q u P and divided by P ONCE ("double hoisting",
 * Bossuat et al., Eurocrypt 2021):   out_o = ModDown(sum_r w_r o sum_d pi_{g_r}(ext_d) o key_{r,d,o}).   An R-term transform runs one ModDown pair instead of R.
 *   accumulate_decomposed : step 3 alone, weighted and accumulating.  d_ext [digits][A][batch][n] (const) and d_keyhat [digits][2][A][n] as for apply_decomposed;
 *                      d_weight [A][weight_batch][n], NTT form under the active primes in that order, words in [0, 4q), weight_batch = batch or 1 (1: one
 *                      weight frame per prime for every frame of the batch); d_weight == NULL means w = 1, and weight_batch is then ignored; d_acc
 *                      [2][A][batch][n] (hoisted_words' apply_scratch_words), the output, read when accumulate = 1 (its old words may be lazy, below 4q).
 *                      Per word, for o = 0, 1, every active slot j with modulus q, every frame f and position i, x' = x mod q:
 *                        t = (sum_d ext_d[j][f][pi_g(i)]' key_{d,o}[j][i]') mod q          -- the word apply_decomposed forms in its scratch
 *                        acc_o[j][f][i] = ((accumulate ? acc_o[j][f][i]' : 0) + w[j][f or 0][i]' t) mod q, fully reduced, exact against big integers:
 *                      w' t + old' < 2^124 + 2^62 is kept in 128 bits and reduced once.  ONE launch on every plan: a streaming kernel, no LDS, no barrier, no
 *                      table; 16-byte accesses when ext, keyhat, acc and the weight are all 16-byte aligned; galois_elt = 1 takes an un-gathered kernel.  No
 *                      inverse tables are needed: a forward-only plan serves.  With d_weight == NULL and accumulate = 0 it is step 3 of apply_decomposed word
 *                      for word (and launches its kernel).
 *   mod_down         : step 4 alone: for o = 0, 1, agx_ntt_basis_mod_down of acc_o with targets Q and sources the special primes, the special slabs of acc_o
 *                      its scratch: they are overwritten, its Q slabs are left unchanged.  acc may hold lazy words; d_out [2][q_count][batch][n], fully
 *                      reduced.  Launches: 2 x what agx_ntt_basis_mod_down_info reports.
 * accumulate_decomposed(w = NULL, accumulate = 0, g) followed by mod_down IS apply_decomposed(g), word for word.  The weight's first q_count slabs are the
 * weight under Q, its last p_count the same plaintext under the special primes.  The sigma_g(c0) terms and an unrotated diagonal join the sum through
 * agx_ntt_mul_add_galois below, after the ModDown ("Linear transforms").
 * Noise.  sum_r w_r acc_r = P M (mod QP) exactly, and the lifts V_o of the special slabs satisfy V_0 + V_1 s = 0 (mod P) with coefficients below
 * p_count P (1 + ||s||_1): what the ONE approximate ModDown leaves is at most p_count (1 + ||s||_1) whatever R and the weights are, where a ModDown per
 * rotation leaves that much multiplied by each weight (tests/test_dhoist_reference.py holds both statements).
 *   Status order of accumulate_decomposed: a NULL ks, ext, keyhat or acc: AGX_ERR_NULL_POINTER; an extent past 2^60 words; weight_batch neither batch nor 1
 *   (with a weight) or accumulate neither 0 nor 1; a pointer not 8-byte aligned, a batch past the grid limit or with A batch above 2^31 - 1, any two of ext /
 *   keyhat / weight / acc touching anywhere (ranges that meet end to end do not touch); galois_elt even, 0 or >= 2n; the plan's device not current:
 *   AGX_ERR_BAD_ARGUMENT, nothing written; batch == 0: AGX_OK, nothing launched.  Of mod_down: NULL; an extent past 2^60 words; alignment, the two grid
 *   limits, acc and out touching anywhere; the device: AGX_ERR_BAD_ARGUMENT; a plan without inverse tables: AGX_ERR_NO_INVERSE; batch == 0: AGX_OK.
 *   Asynchronous on `stream`, allocate and synchronise nothing (capturable into a hipGraph).
 * Measured (profiles/r13_double_hoisting.md, tools/run_op.py --op dhoist; six 60-bit primes, one-frame weights, g = 5 and its powers; (4, 4, 2, 2) at n = 4096 with 4,096
 * frames per prime): an R-term transform by the listing of INTEGRATION.md (decompose, R accumulate_decomposed, ONE mod_down, R mul_add_galois) takes 0.99 / 0.68 / 0.61 of
 * the single-hoisted route's time (decompose, then per rotation apply_decomposed into a temporary and three mul_add_galois) at R = 1 / 4 / 8 -- 14.53 against 23.91 ms at R = 8;
 * over both shapes and n = 4096 / 16384: 0.987 ... 0.995 at R = 1 (level: the spreads overlap in two of the four rows), 0.659 ... 0.688, 0.582 ... 0.615.  One weighted,
 * accumulating call takes 1268 us there: 1.29 of a device copy of its model bytes (1.28 ... 1.36 over the four rows) and 1.64 of agx_ntt_inner_product_galois of the same shape
 * (772 us) -- NOT at the speed of the copy: the weight costs a third product and a second 128-bit reduction per output word, arithmetic and not traffic.  apply and
 * apply_decomposed beside the parent commit's library in the same session: 3433 against 3444 us and 1998 against 1997 us; the spreads overlap in all sixteen pairs of rows.
 * Groups: no group form, as for the other RNS calls. */
AGX_API int agx_ntt_keyswitch_accumulate_decomposed(const agx_ntt_keyswitch* ks, const uint64_t* d_ext, const uint64_t* d_keyhat, const uint64_t* d_weight,
                                                    uint64_t weight_batch, uint64_t* d_acc, uint64_t batch, uint32_t galois_elt, int accumulate, void* stream);
AGX_API int agx_ntt_keyswitch_mod_down(const agx_ntt_keyswitch* ks, uint64_t* d_acc, uint64_t* d_out, uint64_t batch, void* stream);

/* BFV's plaintext boundary on the device: scaling a plaintext modulo t up into Q (encryption, add-plain), its centred lift (multiply-plain), and the rounding
 * round(t X / Q) mod t of decryption in its exact integer RNS form through ONE auxiliary prime gamma (BEHZ: Bajard, Eynard, Hasan, Zucca, SAC 2016, section 3).
 * With them both ends of the BFV pipeline run on library calls at any level of one plan ("BFV encryption, plain operands and decryption").
 * Notation.  Q is the plan primes [q_first, q_first + L), L = q_count <= AGX_BASIS_MAX_SRC = 16; D their product, Q_i = D / q_i; gamma the modulus of plan prime
 * gamma_prime, outside Q (in a BFV multiplication plan any prime of B serves); t the plaintext modulus, 2 <= t < 2^62 -- even, a power of two, composite or above
 * every q_i alike; h = floor(t / 2); centre_gamma(a) = a for a <= (gamma - 1) / 2 and a - gamma above.  All three calls are deterministic integer formulas, exact
 * against big-integer arithmetic.
 *   scale_up    d_m dense [batch][n], ANY 64-bit words, m' = m mod t.  Per coefficient U = floor((2 D m' + t) / (2t)) (D m' / t rounded, halves up) and
 *               out_i = U mod q_i, fully reduced.  d_out dense [L][batch][n], slab i under plan prime q_first + i; AGX_FORM_COEFF: natural order,
 *               AGX_FORM_NTT: NTT_i(out_i) exactly as agx_ntt_forward of the plan writes it.  On the device, with rho = ((D mod t) m' + h) mod t:
 *               U = (D m' + h - rho) / t and, D being 0 modulo q_i, U mod q_i = (h - rho) t^-1 mod q_i: no wide division (csrc/plain_arith.hpp).
 *   lift        operands and forms as scale_up: out_i = m' mod q_i for m' < ceil(t / 2), (m' - t) mod q_i from there on: the centred representative.
 *   scale_down  d_x dense [L][batch][n] in NTT form as agx_ntt_forward / _forward_lazy write it, reduced or lazy; a_i its coefficient form.  Per coefficient
 *                 y_i = a_i' (gamma t Q_i^-1 mod q_i) mod q_i in [0, q_i),    V = sum_i y_i Q_i  (an integer: V = |gamma t X|_D + u D, 0 <= u < L),
 *                 s_t = (-V D^-1) mod t,   s_gamma = (-V D^-1) mod gamma,   c = centre_gamma(s_gamma),   m = (s_t - c) gamma^-1 mod t  in [0, t).
 *               d_m dense [batch][n].  The formula is the contract and is defined for every input.  Property: write t X / D = R + f with R an integer, for ANY
 *               integer X with those residues; then m = R mod t whenever |f| <= 1/2 - L / gamma.  So for a BFV phase X = c_0 + c_1 s (+ c_2 s^2), m is the
 *               message whenever the noise leaves that margin: with a 50- to 60-bit gamma the margin is 1/2 to within 2^-45.
 *               d_scratch: L batch n words; it may be exactly d_x, which is then given up (as agx_ntt_basis_mod_down and agx_ntt_basis_quotient allow);
 *               otherwise it touches d_x nowhere and d_x is left unchanged.  d_m touches neither.
 * Handle.  It belongs to one plan, as a basis does: it holds constants and a pointer to the plan, which must outlive it; the plan's device must be current at
 * creation and at every call; agx_ntt_plan_set_variant between calls stays legal.  The handle type is named by its struct tag, `struct agx_ntt_plain`.
 *   create : NULL: AGX_ERR_NULL_POINTER; q_count == 0 or above 16, a range past P, gamma_prime >= P or inside the range: AGX_ERR_BAD_ARGUMENT; two equal
 *            moduli among Q, gamma equal to a modulus of Q: AGX_ERR_BAD_MODULUS; t < 2 or t >= 2^62: AGX_ERR_BAD_ARGUMENT (the per-word products by t's
 *            constants are Shoup products, which need 2t < 2^64: the bound csrc/bfv_conv_arith.hpp states for its moduli); q_i | t for some i (t needs an
 *            inverse modulo each q_i, D one modulo t), then gamma | t: AGX_ERR_BAD_MODULUS.  On any failure the out-pointer is cleared.
 *   destroy: NULL is fine.
 *   info   : any out-pointer may be NULL; under the plan's CURRENT variant launches_scale_down = the plan's inverse launches + 1 and launches_ntt_form = 1 +
 *            the plan's forward launches.  AGX_FORM_COEFF is ONE launch on every plan.
 * Call rules of all three, agx_ntt_basis_extend_exact's / agx_ntt_basis_quotient's status order: a NULL pointer: AGX_ERR_NULL_POINTER; an unknown form; the
 * plan's device not current; a pointer not 8-byte aligned; a batch past the grid limit or an extent past 2^60 words; an overlap rule broken (scale_up and lift
 * are OUT OF PLACE ONLY; scale_down as above): AGX_ERR_BAD_ARGUMENT, nothing written; scale_down on a plan without inverse tables: AGX_ERR_NO_INVERSE;
 * batch == 0: AGX_OK, nothing launched.  Ranges that meet end to end do not touch.  Asynchronous on `stream`; they allocate and synchronise nothing and touch
 * no plan state (capturable into a hipGraph).
 * Route, one for every plan.  scale_up / lift: ONE streaming kernel, one thread per coefficient (one product modulo t, then one signed Shoup product per
 * prime), 8 (1 + L) bytes per coefficient; AGX_FORM_NTT adds the plan's forward on the view of Q, in place.  scale_down: (1) the plan's inverse on the view of
 * Q into the scratch with n^-1 gamma t Q_i^-1 in the place of n^-1 -- the mechanism of agx_ntt_basis_mod_down's first launch: it writes the y_i itself --,
 * (2) ONE streaming kernel, one thread per coefficient, no LDS, no barrier: the two sums through the rows -q_i^-1 gamma^-1 mod t and -q_i^-1 mod gamma
 * (-Q_i D^-1 = -q_i^-1; gamma^-1 is folded into the t row), the centring, one Shoup product by gamma^-1 mod t, one word stored: 8 (L + 1) bytes per coefficient.
 * Measured (profiles/r17_plain_boundary.md, tools/run_op.py --op plain; 60-bit primes, t = 65537, L = 2, 4, 8, n = 4096 with 4,096 frames per prime and n = 16384 with 1,024, beside a
 * device copy of 8 (L + 1) bytes per coefficient and the plan's transforms alone on the same slabs): scale_up and lift in coefficient form take 0.96 ... 1.12 of the copy's time (L = 4
 * at n = 4096: 126 and 124 us against 125); in NTT form 0.96 ... 1.03 of the plan's forward plus the copy (345 us against 222 + 125).  scale_down takes 1.42 ... 1.52 of the plan's
 * inverse on the same slabs (466 us against 318); less the inverse alone that is 1.12 ... 1.24 of the copy of its kernel's bytes, a difference of two medians: near its traffic, not
 * at it; which of its 2L + 1 products accounts for the rest was not measured.  agx_ntt_basis_quotient and agx_ntt_keyswitch_apply beside the parent commit's library in the same
 * session: 753 / 752 against 747 / 752 us and 3302 / 3294 against 3309 / 3309 us at n = 4096; the spreads overlap in all eight pairs.
 * BGV decryption, the exact centred conversion Q -> t, is agx_ntt_plain_reduce on this handle (section (6), below).  Out of scope: group forms (one
 * handle per shard, as for a basis); a fused NTT-form scale_up. */
struct agx_ntt_plain;
AGX_API int agx_ntt_plain_create(struct agx_ntt_plain** h, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count, uint32_t gamma_prime, uint64_t t);
AGX_API int agx_ntt_plain_destroy(struct agx_ntt_plain* h);
AGX_API int agx_ntt_plain_info(const struct agx_ntt_plain* h, uint32_t* q_first, uint32_t* q_count, uint32_t* gamma_prime, uint64_t* t, int* launches_scale_down,
                               int* launches_ntt_form);
AGX_API int agx_ntt_plain_scale_up(const struct agx_ntt_plain* h, const uint64_t* d_m, uint64_t* d_out, uint64_t batch, int out_form, void* stream);
AGX_API int agx_ntt_plain_lift(const struct agx_ntt_plain* h, const uint64_t* d_m, uint64_t* d_out, uint64_t batch, int out_form, void* stream);
AGX_API int agx_ntt_plain_scale_down(const struct agx_ntt_plain* h, const uint64_t* d_x, uint64_t* d_m, uint64_t* d_scratch, uint64_t batch, void* stream);

/* synthetic coefficients generated on the device: frame (p,b) element i =
 * splitmix64(seed, p, first_poly + b, i) mod q_p, a pure function of its indices (bench / tests) */
AGX_API int agx_ntt_fill_synthetic(const agx_ntt_plan* plan, uint64_t* d_out, uint64_t batch, uint64_t first_poly,
                           uint64_t seed, void* stream);

/* Sampling: the randomness of an encryption or a key, drawn on the device from a 32-byte seed.  Three stateless calls on the plan primes
 * [prime_first, prime_first + prime_count): uniform ring elements (a public `a`: ship the 32 bytes, not the words), ternary secrets and centred-binomial
 * errors.  Exact -- no modulo bias -- and reproducible: a word depends only on (key, nonce, kind, prime index, frame, j), never on batch, launch shape or
 * prime_first.  agx_ntt_fill_synthetic above stays what it is: splitmix64 modulo q, biased, for benchmarks and tests.
 * d_out: dense [prime_count][batch][n], fully reduced, slab i under plan prime prime_first + i.  key: 32 bytes of HOST memory, the caller's seed from its
 * operating system's generator; it is copied into the kernel arguments as eight words and nothing of it is kept after the call.  nonce: the caller's 64-bit
 * draw number, NEVER reused under one key for one kind.  frame_first: the number of the call's first frame in the caller's numbering, so a batch split over
 * several calls or several devices writes the words one call would write (there is no group form, as for a basis).  out_form (ternary, cbd): AGX_FORM_COEFF,
 * or AGX_FORM_NTT = the coefficient launch followed by agx_ntt_forward_range in place on d_out; uniform has no form: uniform NTT-form words are a uniform
 * ring element.
 * The definition.  block(key, w12, w13, w14, w15) is the ChaCha20 block function of RFC 8439 section 2.3, 20 rounds: state words 0..3 the constants, 4..11
 * the key (little-endian), 12..15 as given; o[0..15] its output; the eight 64-bit candidates of a block are c_i = o[2i] | o[2i+1] << 32.  Throughout
 * w13 = F = frame_first + f, w14 = nonce & 0xffffffff, w15 = nonce >> 32.  A cell is eight consecutive coefficients of one frame: c = j >> 3, covering
 * W = min(8, n - 8c) words (for n = 2 and 4 the one cell is the frame); w12 = tag << 16 | c << 4 | k with c < 4096 and k < 16.
 *   uniform, plan prime P (its index in the plan, <= 65534): tag = P, k = the block counter 0..15.  mask = 2^bitlen(q) - 1.  Walk the blocks k = 0, 1, ... and
 *     their candidates i = 0..7 in order; v = c_i & mask is accepted if v < q; the r-th accepted value is word 8c + r; stop when W are accepted.  After block
 *     15 the words still open are written 0 (probability below 2^-90 at acceptance 1/2; acceptance is above 1/2 for every q).
 *   ternary: tag = 0xFFFF, k = 0.  w = c_(j & 7); its fields f_r = (w >> 2r) & 3, r = 0..31; the first field that is not 3 gives 0 -> 0, 1 -> +1, 2 -> -1;
 *     if there is none (probability 2^-64) the value is 0.
 *   cbd: tag = 0xFFFF, k = 1.  w = c_(j & 7); v = popcount(w & (2^eta - 1)) - popcount((w >> 32) & (2^eta - 1)), 1 <= eta <= 32: variance eta / 2 (eta = 21:
 *     sigma = 3.24, the usual error width).
 *   The small kinds write the same v under every prime of the range: v for v >= 0, q + v otherwise (reduced once more under a modulus not above |v|).
 * uniform's running time depends on the rejected candidates only -- public data where `a` is public --; the small kinds are branch-free (a mask and a count of
 * trailing zeros; popcounts).  Out of scope: discrete Gaussians, fixed-Hamming-weight secrets.
 * Status.  NULL plan, key or d_out: AGX_ERR_NULL_POINTER.  A range past the plan's primes or prime_count == 0; frame_first + batch > 2^32; eta outside
 * [1, 32]; an unknown form; the plan's device not current; a pointer not 8-byte aligned, a batch past the grid limit or an extent past 2^60 words:
 * AGX_ERR_BAD_ARGUMENT, nothing written.  batch == 0: AGX_OK, nothing launched.  Asynchronous on `stream`; they allocate and synchronise nothing and touch no
 * plan state (capturable into a hipGraph).
 * Route.  ONE streaming launch each, no table, no LDS, no barrier: one thread per cell, the sixteen working words in vector registers, the key, the
 * constants and the nonce in scalar registers, a lane's 64 contiguous bytes stored 16 at a time where d_out is 16-byte aligned.  uniform: one row of the
 * grid per prime; the small kinds compute a cell's eight values once and walk the primes.  Measured: profiles/r19_sampling.md. */
AGX_API int agx_ntt_sample_uniform(const agx_ntt_plan* plan, const uint8_t key[32], uint64_t nonce, uint64_t* d_out, uint64_t batch, uint64_t frame_first,
                                   uint32_t prime_first, uint32_t prime_count, void* stream);
AGX_API int agx_ntt_sample_ternary(const agx_ntt_plan* plan, const uint8_t key[32], uint64_t nonce, uint64_t* d_out, uint64_t batch, uint64_t frame_first,
                                   uint32_t prime_first, uint32_t prime_count, int out_form, void* stream);
AGX_API int agx_ntt_sample_cbd(const agx_ntt_plan* plan, const uint8_t key[32], uint64_t nonce, uint32_t eta, uint64_t* d_out, uint64_t batch,
                               uint64_t frame_first, uint32_t prime_first, uint32_t prime_count, int out_form, void* stream);

/* ------------------------------------------------------------------------- */
/* (4) Host math the reference leaves to its caller (src/main.cpp:49-55 ships   */
/* placeholders only).                                                          */
/* ------------------------------------------------------------------------- */
/* the `count` largest primes q < 2^bits with q = 1 (mod 2n), descending */
AGX_API int agx_ntt_find_primes(uint32_t bits, uint32_t n, uint32_t count, uint64_t* primes_out);
AGX_API int agx_ntt_min_root(uint64_t q, uint32_t n, uint64_t* psi_out);
AGX_API int agx_ntt_make_tables(uint64_t q, uint64_t psi, uint32_t n, uint64_t* twiddles, uint64_t* precons);
AGX_API int agx_ntt_make_inverse_tables(uint64_t q, uint64_t psi, uint32_t n, uint64_t* inv_twiddles, uint64_t* inv_precons);
/* the Galois element of a slot rotation by `step`: g = 5^step mod 2n, a negative step taking powers of 5^-1 mod 2n; always odd and below 2n.
 * (Conjugation is not a power of 5: its element is g = 2n - 1.)  Pure arithmetic, no device needed */
AGX_API int agx_ntt_galois_element(uint32_t n, int64_t step, uint32_t* galois_elt);

/* CKKS encoding and decoding on the device: a vector of complex slots <-> a plaintext polynomial in RNS form, the canonical-embedding ("special") FFT over the
 * rotation group fused with the double <-> RNS conversions, one frame per workgroup.  With them a CKKS pipeline runs on library calls end to end
 * ("CKKS encode, encrypt, multiply-plain, rescale, rotate, decrypt, decode"), and the slot order is stated once, here.
 * Notation.  n the plan's size, M = 2n; slots = s, a power of two with 1 <= s <= n / 2; gap = (n / 2) / s; count = l with 1 <= l <= q_count: a call works on the
 * plan primes [q_first, q_first + l), a PREFIX of the handle's range (a CKKS level drops primes from the end, so one handle serves every level); D the product
 * of those l primes; Delta = scale, any finite double > 0.
 * Layouts.  d_z dense [batch][s] of (re, im) pairs of doubles, 8-byte aligned; d_out and d_x dense [l][batch][n], slab i under plan prime q_first + i.
 * The transform in closed form, zeta' = exp(i pi / (2s)):
 *   decode  z_j = (1 / Delta) sum_{k < 2s} X_{k gap} zeta'^(5^j k), j < s, X the centred representative modulo D; coefficients off the gap grid are ignored.
 *   encode  w_k = (1 / s) sum_{j < s} z_j zeta'^(-5^j k), k < s;  X_{k gap} = rint(Delta Re w_k), X_{(k + s) gap} = rint(Delta Im w_k), every other coefficient 0.
 * Slot j sits at the root zeta^(5^j): agx_ntt_automorphism with g = agx_ntt_galois_element(n, r) rotates full slots left by r, g = 2n - 1 conjugates them.
 * The definition is a fixed operation graph in IEEE double; no step is contracted or reassociated, so a float64 model that follows it gives the same bits
 * (tests/ckks_ref.py), and the definition is the contract, word for word.
 *   Twiddles.  tw(len, j) = (cos theta, sin theta), theta = 2 pi (5^j mod 4 len) / (4 len): what agx_ntt_ckks_twiddle returns, for len a power of two in
 *     [2, 16384] and j < len / 2 (anything else, AGX_ERR_BAD_ARGUMENT; out NULL: AGX_ERR_NULL_POINTER).  Each component within 2^-53 absolute of the real
 *     value: the angle is reduced exactly in integers to an octant, cosine and sine taken in long double and rounded once.  The value depends on neither n
 *     nor s: one table of n / 2 - 1 entries, indexed len / 2 + j, serves every slot count.
 *   Complex arithmetic.  a b = (a_r b_r - a_i b_i, a_r b_i + a_i b_r): four products, two sums.  The conjugate twiddle is (cos theta, -sin theta).
 *   Decode core (forward special FFT).  v_k = (x_k, x_{k+s}) for k < s, x the doubles below; bit-reverse v; for len = 2, 4, ..., s, every block start i and
 *     every j < len / 2:  u = v[i+j], w = v[i+j+len/2] tw(len, j), v[i+j] = u + w, v[i+j+len/2] = u - w;  z_j = v_j (1 / Delta): one product per component by
 *     the double 1 / Delta.
 *   Encode core (inverse special FFT).  v = z; for len = s, s / 2, ..., 2:  u = v[i+j] + v[i+j+len/2], w = (v[i+j] - v[i+j+len/2]) conj tw(len, j), stored in
 *     their places; bit-reverse; multiply by 1 / s (exact); x = fl(Delta component); c = rint(x), ties to even, a non-finite x giving c = 0; the residue is
 *     c mod q_i in [0, q_i), for ANY finite double: from |x| = 2^63 on x is an integer mant 2^e with mant its 53-bit significand, and the residue is
 *     mant (2^e mod q_i) mod q_i, the second factor from a table that only those words index past its first entry.
 *   RNS -> double (decode's input).  (1) The mixed-radix (Garner) digits of X mod D = v_1 + v_2 q_1 + v_3 q_1 q_2 + ..., v_i in [0, q_i), exact, with
 *     word-size Shoup products.  (2) X is negative iff (v_l, ..., v_1) is greater than ((q_l - 1) / 2, ..., (q_1 - 1) / 2) compared from the top: those are
 *     exactly the digits of (D - 1) / 2.  (3) For a negative X the magnitude digits are q_i - 1 - v_i, plus 1 with a carry from the bottom.  (4) Horner from the
 *     top in double: acc = (double)w_l, then acc = acc (double)q_i + (double)w_i for i = l - 1 down to 1, every conversion rounding to nearest even.  (5) The
 *     sign.  The Garner constants of a prefix are a prefix of the handle's triangular table.
 * Handle.  It belongs to one plan, as a basis does: it holds tables (the twiddles, the Garner constants, 2^e mod q_i for e < 1024) and a pointer to the plan,
 * which must outlive it; the plan's device must be current at creation and at every call; agx_ntt_plan_set_variant between calls stays legal.  The handle type
 * is named by its struct tag, `struct agx_ntt_ckks`.
 *   create : NULL: AGX_ERR_NULL_POINTER; q_count == 0 or above AGX_BASIS_MAX_SRC = 16, a range past P: AGX_ERR_BAD_ARGUMENT; two equal moduli in the range:
 *            AGX_ERR_BAD_MODULUS.  On any failure the out-pointer is cleared.
 *   destroy: NULL is fine.
 *   info   : any out-pointer may be NULL; max_slots = n / 2; under the plan's CURRENT variant launches_encode_ntt = 1 + the plan's forward launches and
 *            launches_decode_ntt = the plan's inverse launches + 1.  AGX_FORM_COEFF is ONE launch on every plan, both ways.
 * Call rules, agx_ntt_plain_*'s status order: a NULL pointer (decode's d_scratch only in NTT form): AGX_ERR_NULL_POINTER; count == 0 or above q_count; slots
 * not a power of two in [1, n / 2]; scale not finite or <= 0; an unknown form; the plan's device not current; a pointer not 8-byte aligned; a batch past the
 * grid limit or an extent past 2^60 words; encode: d_z touching d_out; decode: d_z touching d_x or the scratch, the scratch touching d_x without being d_x:
 * AGX_ERR_BAD_ARGUMENT, nothing written; NTT-form decode on a plan without inverse tables: AGX_ERR_NO_INVERSE; batch == 0: AGX_OK, nothing launched.
 * Asynchronous on `stream`; they allocate and synchronise nothing and touch no plan state (capturable into a hipGraph).
 * Routes.  encode: ONE kernel does the FFT, the rounding and all l residues, 16 s + 8 n l bytes per frame; AGX_FORM_NTT adds agx_ntt_forward_range in place on
 * d_out.  decode: with AGX_FORM_NTT the plan's inverse runs on the range into d_scratch (l batch n words; it may be exactly d_x, which is then given up,
 * agx_ntt_plain_scale_down's rules; the input may be reduced or lazy), then ONE kernel does Garner, the FFT and the store; AGX_FORM_COEFF takes fully reduced
 * words, is one launch, never looks at d_scratch (it may be NULL) and leaves d_x unchanged.
 * Kernel shape (csrc/ckks_kernels.hpp).  One workgroup per frame, s / 4 threads within [64, 1024]; register-blocked radix-8 passes (a thread holds eight
 * complex values at one stride and does three stages on them; the last pass takes what is left), a workgroup barrier between passes; the exchange goes through
 * LDS as separate real and imaginary planes of s doubles: up to s = 8192, 128 KiB.  s = 16384 (n = 32768, full slots, 256 KiB) takes another route: the same
 * passes exchange through the frame's own output words in global memory (decode: its d_z frame; encode: its frame of slab 0, whose n words are s pairs of
 * doubles), which no other workgroup touches, and encode moves every component off those words (the real ones into LDS, the imaginary ones into registers) and passes
 * one more barrier before the residues overwrite them.  The grouping of stages into passes changes no bit: the radix-2 graph fixes every rounding.
 * Measured (profiles/r20_ckks_boundary.md, tools/run_op.py --op ckks; full slots, Delta = 2^40, l = 1, 2, 4 60-bit primes, n = 4096 with 4,096 frames and n = 16384 with 1,024,
 * beside a device copy of 16 s + 8 n l bytes per frame and the plan's transforms alone on the same slabs): in coefficient form encode takes 1.76 ... 4.19 and decode 1.73 ... 3.73 of
 * the copy's time (l = 4 at n = 4096: 218 and 247 us against 124), the ratios falling as l grows for encode; both are bound by the FFT's passes and, decode at l = 4, by Garner's
 * O(l^2) products, not by their traffic.  In NTT form encode takes 1.18 ... 1.90 of the plan's forward plus the copy, decode 1.16 ... 1.56 of the plan's inverse plus the copy.
 * Out of scope: group forms; more than 16 primes per handle (two handles serve a longer chain); real-only or conjugate-invariant packings. */
struct agx_ntt_ckks;
AGX_API int agx_ntt_ckks_create(struct agx_ntt_ckks** h, const agx_ntt_plan* plan, uint32_t q_first, uint32_t q_count);
AGX_API int agx_ntt_ckks_destroy(struct agx_ntt_ckks* h);
AGX_API int agx_ntt_ckks_info(const struct agx_ntt_ckks* h, uint32_t* q_first, uint32_t* q_count, uint32_t* max_slots, int* launches_encode_ntt,
                              int* launches_decode_ntt);
AGX_API int agx_ntt_ckks_encode(const struct agx_ntt_ckks* h, const double* d_z, uint32_t slots, double scale, uint64_t* d_out, uint64_t batch, uint32_t count,
                                int out_form, void* stream);
AGX_API int agx_ntt_ckks_decode(const struct agx_ntt_ckks* h, const uint64_t* d_x, int in_form, uint32_t count, double scale, double* d_z, uint32_t slots,
                                uint64_t* d_scratch, uint64_t batch, void* stream);
AGX_API int agx_ntt_ckks_twiddle(uint32_t len, uint32_t j, double out[2]);

/* ------------------------------------------------------------------------- */
/* (5) Groups: the same calls over several GPUs of one node.                    */
/* The reference deals the frames of a call to its replicated compute units     */
/* inside the call: unit i gets floor(F / C) + [i < F mod C] frames             */
/* (src/kernel/ntt.cpp:526-536), frame b goes to unit b % C (:579-582) and is   */
/* collected from it (:622-625); units never exchange data.  A group is that    */
/* scheme over whole devices: one SHARD per entry of `devices` (a device may be */
/* listed more than once), each with its own plan (tables prepared once on the  */
/* host), stream, staging buffers and host thread.  Frames are dealt in          */
/* CONTIGUOUS blocks of the reference's minibatch sizes (agx_ntt_shard_range).   */
/* No collective, no peer access: nothing is exchanged between shards.           */
/* A bad device id returns AGX_ERR_BAD_ARGUMENT; a call's status is that of the  */
/* lowest-numbered failing shard.  One call at a time per group (calls from      */
/* several host threads serialise).                                               */
/* ------------------------------------------------------------------------- */
typedef struct agx_ntt_group agx_ntt_group;

/* block of shard `index` when num_frames frames are dealt to num_shards shards: pure arithmetic, no device needed */
AGX_API int agx_ntt_shard_range(uint64_t num_frames, uint32_t num_shards, uint32_t index, uint64_t* first, uint64_t* count);

/* arguments after num_devices as agx_ntt_plan_create / agx_ntt_plan_create_auto */
AGX_API int agx_ntt_group_create(agx_ntt_group** group, const int* devices, uint32_t num_devices, uint32_t n, uint32_t num_primes,
                                 const uint64_t* moduli, const uint64_t* twiddles, const uint64_t* precons,
                                 const uint64_t* inv_twiddles, const uint64_t* inv_precons);
AGX_API int agx_ntt_group_create_auto(agx_ntt_group** group, const int* devices, uint32_t num_devices, uint32_t n, uint32_t num_primes,
                                      const uint64_t* moduli, const uint64_t* psi);
AGX_API int agx_ntt_group_destroy(agx_ntt_group* group);
AGX_API int agx_ntt_group_info(const agx_ntt_group* group, uint32_t* num_shards, uint32_t* n, uint32_t* num_primes);
/* shard `index`: its device, its plan (owned by the group) and its stream (a hipStream_t: record events on it to time a shard) */
AGX_API int agx_ntt_group_shard(const agx_ntt_group* group, uint32_t index, int* device, agx_ntt_plan** plan, void** stream);

/* host frames (one modulus): agx_ntt_forward_host_stream / agx_ntt_inverse_host_stream on every shard's block at once, each shard */
/* from its own host thread through its own three-slot pipeline; synchronous                                                       */
AGX_API int agx_ntt_group_forward_host(const agx_ntt_group* group, const uint64_t* in, const uint64_t* in2, uint64_t* out, uint64_t num_frames);
AGX_API int agx_ntt_group_inverse_host(const agx_ntt_group* group, const uint64_t* in, uint64_t* out, uint64_t num_frames);

/* device pointers: arrays with one entry per shard -- d_in[i] / d_out[i] live on shard i's device in the dense [prime][batch[i]][n] */
/* layout.  Every shard is launched from its own host thread on its own stream; the call returns when every launch has been queued  */
/* (asynchronous like agx_ntt_forward); agx_ntt_group_synchronize waits for all shards' streams.                                    */
AGX_API int agx_ntt_group_forward(const agx_ntt_group* group, const uint64_t* const* d_in, uint64_t* const* d_out, const uint64_t* batch);
AGX_API int agx_ntt_group_inverse(const agx_ntt_group* group, const uint64_t* const* d_in, uint64_t* const* d_out, const uint64_t* batch);
/* d_scratch may be NULL (or hold NULL entries) wherever agx_ntt_polymul accepts a NULL scratch */
AGX_API int agx_ntt_group_polymul(const agx_ntt_group* group, const uint64_t* const* d_a, const uint64_t* const* d_b, uint64_t* const* d_c,
                                  uint64_t* const* d_scratch, const uint64_t* batch);
/* agx_ntt_polymul_ntt per shard; bhat_batch[i] is batch[i] or 1 */
AGX_API int agx_ntt_group_polymul_ntt(const agx_ntt_group* group, const uint64_t* const* d_a, const uint64_t* const* d_bhat,
                                      uint64_t* const* d_c, const uint64_t* batch, const uint64_t* bhat_batch);
/* agx_ntt_rescale per shard; every shard needs its own scratch (which may be its d_x's last slab) */
AGX_API int agx_ntt_group_rescale(const agx_ntt_group* group, const uint64_t* const* d_x, uint64_t* const* d_out,
                                  uint64_t* const* d_scratch, const uint64_t* batch, int mode);
/* agx_ntt_automorphism per shard, the same Galois element and form on every shard */
AGX_API int agx_ntt_group_automorphism(const agx_ntt_group* group, const uint64_t* const* d_in, uint64_t* const* d_out, const uint64_t* batch,
                                       uint32_t galois_elt, int form);
AGX_API int agx_ntt_group_synchronize(const agx_ntt_group* group);

/* ------------------------------------------------------------------------- */
/* (6) BFV / BGV from slots to slots: batching and exact BGV decryption.       */
/* ------------------------------------------------------------------------- */
/* A. SIMD batching for the integer schemes: a vector of n slots modulo t <-> the plaintext polynomial m that agx_ntt_plain_scale_up / _lift take and that
 * agx_ntt_plain_scale_down / _reduce give back ("BFV with batching" and "BGV").  The slot order is the one that makes the rotations of
 * agx_ntt_automorphism rotate: it is stated here, once, for the integer schemes, as the CKKS block above states it for CKKS.
 * Definition (the contract, word for word).  M = 2n; t is prime, t = 1 (mod M), t < 2^62; psi = agx_ntt_min_root(t, n), which info returns.  Exponents:
 * e_j = 5^j mod M for j < n / 2, and e_{n/2+j} = M - e_j.
 *   decode  z_j = m(psi^{e_j}) mod t for j < n.  Input words lie in [0, t), as agx_ntt_plain_scale_down and agx_ntt_plain_reduce write them; larger words give
 *           unspecified values and never an out-of-range access: no index is formed from data.
 *   encode  the inverse of decode: d_z words are taken modulo t (ANY 64-bit word is accepted), d_m is written in [0, t).
 * Layouts are dense [batch][n].  Slots 0 ... n / 2 - 1 are row 0, the rest are row 1.  In the library's NTT order (out[brev(k)] = x(psi^{2k+1}), brev over
 * log2 n bits) slot j sits at word pos(j) = brev((e_j - 1) / 2).
 * Properties.  (1) Slot-wise ring homomorphism: the slots of m + m' and of m m' mod (X^n + 1, t) are the slot-wise sums and products.  (2) sigma_g: X -> X^g
 * with g = agx_ntt_galois_element(n, r) rotates BOTH rows left by r: the new slot j of a row is its old slot j + r mod n / 2 (e_j g = e_{j+r}).  (3) g = 2n - 1
 * swaps the rows (e_j (M - 1) = M - e_j).  They hold for a ciphertext's plaintext as for m itself, so agx_ntt_automorphism and the hoisted rotations rotate slots.
 * Handle.  It owns a one-prime plan under t on the device current at creation (agx_ntt_plan_create_auto(n, 1, &t, &psi), with inverse tables) -- NOT a prime of
 * the caller's plan: a 17-bit t among 2^60 - c primes would take that plan off its specialised class -- and two uint32 index tables of n entries on the device,
 * slot -> word and word -> slot, built once on the host.  That device must be current at every call.  The handle type is named by its struct tag.
 *   create : NULL: AGX_ERR_NULL_POINTER; n not a size the plans admit: AGX_ERR_BAD_ARGUMENT; t composite, t != 1 (mod 2n) or t >= 2^62: AGX_ERR_BAD_MODULUS.
 *            On any failure the out-pointer is cleared.
 *   destroy: NULL is fine.
 *   info   : any out-pointer may be NULL; launches_encode = 1 + the inner plan's inverse launches and launches_decode = the inner plan's forward launches + 1,
 *            under the inner plan's CURRENT variant.
 *   plan   : lends the inner plan, which the handle owns (never destroy it): for plaintext-side products modulo t and for agx_ntt_plan_set_variant.
 * Call rules, agx_ntt_plain_*'s status order: a NULL pointer: AGX_ERR_NULL_POINTER; the handle's device not current; a pointer not 8-byte aligned; a batch past
 * the grid limit or an extent past 2^60 words; an overlap rule broken: AGX_ERR_BAD_ARGUMENT, nothing written; batch == 0: AGX_OK, nothing launched.  d_z and d_m
 * never touch each other.  decode's d_scratch (batch n words) may be exactly d_m, which is then given up (agx_ntt_plain_scale_down's rule); otherwise it touches
 * d_m nowhere and d_m is left unchanged; d_z touches neither.  Asynchronous on `stream`; the calls allocate nothing and are capturable into a hipGraph.
 * Routes.  encode: ONE streaming kernel (csrc/batch_kernels.hpp; it reads d_z through the word -> slot table, reduces modulo t by a precomputed reciprocal and
 * writes d_m in contiguous runs), then the inner plan's inverse in place on d_m.  decode: the inner plan's forward from d_m into d_scratch, then the same kernel
 * the other way: it reads d_scratch through slot -> word and writes d_z contiguously.  The kernel: no LDS, no barrier, the table read coalesced, grid-stride,
 * 16-byte stores where the output is 16-byte aligned.  The READ is the gathered side in both directions, by the measurement below.
 * Measured (profiles/r21_batching.md, tools/run_op.py --op batch; t = 65537, n = 4096 with 4,096 frames and n = 16384 with 1,024, beside the inner plan's transforms alone
 * and a device copy of the permutation's 16 n bytes per frame): encode 135 us against an inner inverse of 52 and a copy of 32.5 at n = 4096, 237 against 59 and 32.7 at
 * n = 16384; decode 133 against a forward of 48.6, and 217 against 50.  The permutation kernel (a call less its transform, a difference of two medians) takes 2.5 ... 2.6
 * of the copy at n = 4096 and 5.1 ... 5.5 at n = 16384, far outside the copy's spread (under 2 %).  The gathered side was chosen by a number: the same kernel with
 * contiguous 16-byte loads and scattered 8-byte writes (an A/B library built with -DAGX_BATCH_SCATTER, the two alternating in one session, two rounds) takes 4.1 of the
 * copy for encode and 5.8 for decode at n = 4096 (133 and 188 us against 82 and 84), and 5.4 and 9.1 at n = 16384 (178 and 302 us against 176 and 167): gathered reads
 * win or tie in all eight pairs and ship for both directions.  With equal bytes the side that moves 8 bytes at a bit-reversed stride decides the time, and the cost per
 * word doubles from a 32 KiB frame to a 128 KiB one: that fits a bound on L2 sector traffic of the 8-byte accesses; no counter was collected to prove it.
 *
 * B. BGV decryption on the plaintext handle of section agx_ntt_plain_* above: the exact centred conversion Q -> t.
 *   reduce  d_x dense [L][batch][n] in NTT form, reduced or lazy; X the representative of its coefficient form in [-(D - 1) / 2, (D - 1) / 2].  Per coefficient
 *           m = (factor mod t) X mod t, in [0, t); d_m dense [batch][n].  Exact for every input and for EVERY t that agx_ntt_plain_create admits, even ones
 *           included: no inverse modulo t is used.  factor = 1 is plain decryption (a BGV phase X = m + t e decrypts to m while |X| <= (D - 1) / 2);
 *           factor = D_dropped mod t undoes the D_dropped^-1 mod t that agx_ntt_basis_mod_down_mode leaves in a BGV plaintext.
 *           Scratch and overlap rules, status order and AGX_ERR_NO_INVERSE are agx_ntt_plain_scale_down's.  The handle's gamma_prime stays a required argument
 *           of create and is not used by this call.
 * Route.  The plan's inverse on the view of Q into the scratch (its own constants), then ONE streaming kernel, one thread per coefficient: the Garner digits
 * v_i of X mod D (the steps of CKKS decode, csrc/ckks_arith.hpp), the sign by comparing them from the top with the digits (q_i - 1) / 2 of (D - 1) / 2, then
 * sum_i v_i (prod_{k<i} q_k mod t) - [negative] (D mod t) modulo t, then one Shoup product by factor mod t, whose reciprocal the host forms per call.
 * Measured (profiles/r21_batching.md; 60-bit primes, t = 65537, beside agx_ntt_plain_scale_down on the same slabs): 0.95 ... 0.99 of scale_down at L = 2 (245 us against
 * 259 at n = 4096), 1.19 at L = 4 (560 against 472), 1.53 ... 1.57 at L = 8 (1415 against 903): less the plan's inverse, the kernel is at 1.05 ... 1.17 of a copy of its
 * 8 (L + 1) bytes per coefficient at L = 2 and compute-bound from L = 4 on, by Garner's L (L - 1) products.  agx_ntt_keyswitch_apply and agx_ntt_plain_scale_down
 * beside the parent commit's library in the same session, two rounds: 3257.8 / 3257.7 against 3256.2 / 3258.6 us and 463.5 / 462.6 against 461.5 / 464.1 us at
 * n = 4096; the spreads overlap in all pairs.  Every kernel of the parent is textually identical in this tree (profiles/r21_batching_device_asm.txt).
 * Out of scope: group forms (one handle per shard). */
struct agx_ntt_batch;
AGX_API int agx_ntt_batch_create(struct agx_ntt_batch** h, uint32_t n, uint64_t t);
AGX_API int agx_ntt_batch_destroy(struct agx_ntt_batch* h);
AGX_API int agx_ntt_batch_info(const struct agx_ntt_batch* h, uint32_t* n, uint64_t* t, uint64_t* psi, int* launches_encode, int* launches_decode);
AGX_API int agx_ntt_batch_plan(const struct agx_ntt_batch* h, agx_ntt_plan** plan);
AGX_API int agx_ntt_batch_encode(const struct agx_ntt_batch* h, const uint64_t* d_z, uint64_t* d_m, uint64_t batch, void* stream);
AGX_API int agx_ntt_batch_decode(const struct agx_ntt_batch* h, const uint64_t* d_m, uint64_t* d_z, uint64_t* d_scratch, uint64_t batch, void* stream);
AGX_API int agx_ntt_plain_reduce(const struct agx_ntt_plain* h, const uint64_t* d_x, uint64_t* d_m, uint64_t* d_scratch, uint64_t factor, uint64_t batch,
                                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AGX_NTT_H */
