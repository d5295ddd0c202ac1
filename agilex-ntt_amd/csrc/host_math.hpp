// host_math.hpp -- host-side number theory for plan creation: NTT-friendly primes,
// primitive roots and the twiddle / precomputed-quotient tables the reference expects its
// caller to provide (include/kernel/ntt.h:35-41; src/main.cpp:49-55 ships placeholders only).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace agx {

uint64_t mul_mod(uint64_t a, uint64_t b, uint64_t q);
uint64_t pow_mod(uint64_t a, uint64_t e, uint64_t q);
uint64_t inv_mod(uint64_t a, uint64_t q);  // q prime
bool inv_mod_euclid(uint64_t a, uint64_t q, uint64_t* inv);  // any q > 1: false when gcd(a, q) != 1
bool is_prime_u64(uint64_t q);
inline bool is_pow2(uint32_t n) { return n && !(n & (n - 1)); }
inline int log2u(uint32_t n) { int l = 0; while ((1u << l) < n) ++l; return l; }
inline uint32_t bit_reverse(uint32_t x, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) { r = (r << 1) | (x & 1u); x >>= 1; }
    return r;
}

// descending list of primes below 2^bits congruent to 1 mod 2n
std::vector<uint64_t> find_ntt_primes(uint32_t bits, uint32_t n, uint32_t count);
// least primitive 2n-th root of unity mod q, 0 if q-1 is not divisible by 2n
uint64_t min_primitive_root_2n(uint64_t q, uint32_t n);
bool is_primitive_root_2n(uint64_t psi, uint64_t q, uint32_t n);

// floor(w * 2^64 / q), w < q
uint64_t shoup_quotient(uint64_t w, uint64_t q);
// tw[j] = base^bitrev(j) mod q, pre[j] = shoup_quotient(tw[j])
void power_tables_bitrev(uint64_t q, uint64_t base, uint32_t n, uint64_t* tw, uint64_t* pre);

// The table entry of the two-twiddle butterfly for q = 2^60 - c, 0 < c < 2^28 (csrc/modarith.hpp: ct_butterfly_q60c_fold), from a twiddle
// w < q alone: wC = w 2^32 mod q, and each of the two split at bit 29 into the words of one 64-bit value --
//   w_packed = (w mod 2^29) | (w >> 29) << 32,   wc_packed = (wC mod 2^29) | (wC >> 29) << 32;   the high halves are below 2^31.
struct fold_twiddle {
    uint64_t w_packed, wc_packed;
};
fold_twiddle fold_twiddle_pack(uint64_t w, uint64_t q);

// A word w < q with its precomputed quotient floor(w 2^64 / q): what one Shoup product reads.  The device reads it as a ulonglong2 (plan_internal.hpp
// asserts size and alignment).
struct alignas(16) shoup_pair {
    uint64_t w, p;
    static shoup_pair of(uint64_t w, uint64_t q) { return {w, shoup_quotient(w, q)}; }
};

// h mod q for h = floor(D / 2), D = prod src[i] odd, q odd and > 1: h is a multi-word integer (S up to 16 moduli of 62 bits) and is never formed.
// 2 h = D - 1 exactly, so h = (D - 1) 2^-1 (mod q) with 2^-1 = (q + 1) / 2; D mod q is taken one factor at a time in 128 bits, or is the caller's.
uint64_t half_product_mod(const uint64_t* src, uint32_t S, uint64_t q);
uint64_t half_product_mod(uint64_t d_mod_q, uint64_t q);

// What a basis is asked for: a fast RNS base conversion from the moduli src[0 .. S) to the moduli dst[0 .. T), every modulus odd, > 1 and < 2^62.
struct basis_request {
    const uint64_t* src;
    uint32_t S;
    const uint64_t* dst;
    uint32_t T;
    const uint64_t *n_inv, *w1n;      // [S]: the two constants of an inverse transform's last stage, n^-1 mod src[i] and inv_twiddle[1] n^-1 mod src[i], both below src[i]
    uint64_t t = 1;                   // the plaintext modulus of agx_ntt_basis_create_plain: any 64-bit value, reduced per modulus here
    uint64_t m = 0;                   // the auxiliary modulus of agx_ntt_basis_create_aux, odd, > 1 and < 2^62; 0: none
    // agx_ntt_basis_create_quotient only (it needs an m): quot_t != 0 asks for the quotient's constants.  The quotient runs the inverse on the TARGETS
    // and on m as well, so it needs their last-stage constants: dst_n_inv, dst_w1n [T] and the two of m, as n_inv and w1n are the sources'.
    uint64_t quot_t = 0;              // the t of the quotient: any 64-bit value, reduced per modulus here; 0: no quotient
    const uint64_t *dst_n_inv = nullptr, *dst_w1n = nullptr;
    uint64_t aux_n_inv = 0, aux_w1n = 0;
};

// Everything a basis keeps on the device, built once on the host.  With D = prod src[i], D_i = D / src[i], q_i = src[i], q_j = dst[j], every pair
// {word, its quotient for the modulus the word is reduced by}:
struct basis_image {
    // agx_ntt_basis_extend
    std::vector<shoup_pair> dinv;      // [S]    D_i^-1 mod q_i
    std::vector<shoup_pair> mat;       // [T][S] D_i mod q_j.  A target that is itself source k gets 0 for i != k, so the conversion hands that residue through.
    // agx_ntt_basis_mod_down
    std::vector<shoup_pair> dall;      // [T]    D^-1 mod q_j -- {0, 0} where D is not invertible modulo q_j (q_j shares a factor with a source; for primes: equals one)
    bool moddown_legal = false;        // every dall[j] exists
    // [S]: n_inv[i] t^-1 D_i^-1 mod q_i and w1n[i] t^-1 D_i^-1 mod q_i, the last stage's constants scaled so that the inverse of the source slabs writes
    // y_i = p_i t^-1 D_i^-1 mod q_i itself.  With t = 1 they are n_inv[i] D_i^-1 and w1n[i] D_i^-1: nothing changes.
    std::vector<shoup_pair> sn, sw;
    std::vector<shoup_pair> down_mat;  // [T][S] t D_i mod q_j: ModDown's matrix, a copy of its own (agx_ntt_basis_extend keeps mat); with t = 1 the words of mat
    // the two constant sets of AGX_RESCALE_ROUND (csrc/moddown_arith.hpp), h = floor(D / 2)
    std::vector<shoup_pair> round_src; // [S]    {c_i = h D_i^-1 mod q_i, q_i}: the second word is the modulus, not a quotient
    std::vector<uint64_t> round_dst;   // [T]    t h mod q_j
    // agx_ntt_basis_extend_exact and agx_ntt_basis_extend_mont (csrc/bfv_conv_arith.hpp has the formulas): filled when the request has an m, else empty
    std::vector<shoup_pair> aux_row;         // [S]    D_i mod m
    std::vector<shoup_pair> aux_corr_exact;  // [T]    D mod q_j
    std::vector<shoup_pair> aux_mdinv;       // [S]    m D_i^-1 mod q_i
    std::vector<shoup_pair> aux_mmat;        // [T][S] D_i m^-1 mod q_j
    std::vector<shoup_pair> aux_corr_mont;   // [T]    -D m^-1 mod q_j
    shoup_pair k_exact = {0, 0}, k_mont = {0, 0};      // D^-1 mod m, -D^-1 mod m
    // agx_ntt_basis_quotient (csrc/bfv_quotient_arith.hpp has the formulas): filled when the request has a quot_t, else empty.  The quotient divides by the
    // product of the TARGETS, E = prod q_j, E_j = E / q_j, and returns through the sources: D, D_i and m are the above.  The scaled last-stage constants
    // make the inverse of the target slabs write y_j = t a_j E_j^-1 mod q_j and the inverse of the source slabs and of m's write s_i = t a_i E^-1 D_i^-1
    // mod q_i and s_m = t a_m E^-1 mod m.
    std::vector<shoup_pair> quot_dn, quot_dw;  // [T]     dst_n_inv[j] t E_j^-1 mod q_j and dst_w1n[j] t E_j^-1 mod q_j
    std::vector<shoup_pair> quot_sn, quot_sw;  // [S + 1] n_inv[i] t E^-1 D_i^-1 mod q_i and w1n[i] t E^-1 D_i^-1 mod q_i; entry S: aux_n_inv t E^-1 mod m, aux_w1n t E^-1 mod m
    std::vector<shoup_pair> quot_mat;          // [T][S + 1] q_j^-1 D_i^-1 mod q_i (= E_j E^-1 D_i^-1); column S: q_j^-1 mod m
};

// Which rule refused a request, the first in this order; nothing is promised about the image then.
enum class basis_fault {
    none,
    source,      // some D_i is not invertible modulo src[i]: two source moduli share a factor (for primes: are equal)
    t,           // t has no inverse modulo some source (for prime sources: t = 0 modulo one of them)
    aux,         // D has no inverse modulo m, or m none modulo some target (for primes: m equals a source or a target)
    quotient,    // some E_j has no inverse modulo its target, or E none modulo a source or m (for primes: two targets are equal, or a target is a source or m)
};
basis_fault prepare_basis_image(basis_image& img, const basis_request& rq);

// What a plaintext boundary (agx_ntt_plain_*) is asked for: Q = the moduli q[0 .. L), every one odd, > 1 and < 2^62, the auxiliary modulus gamma of the same
// kind, the plaintext modulus t in [2, 2^62) -- even, a power of two, composite or above every q[i] alike -- and the two last-stage constants of an inverse
// transform per q[i], as a basis_request carries them.
struct plain_request {
    const uint64_t* q;
    uint32_t L;
    const uint64_t *n_inv, *w1n;      // [L], both below q[i]
    uint64_t gamma, t;
};

// Everything such a handle keeps on the device or hands to its kernels, built once on the host (csrc/plain_arith.hpp has the formulas).  With D = prod q[i]
// and Q_i = D / q[i], every pair {word, its quotient for the modulus the word is reduced by}:
struct plain_image {
    std::vector<shoup_pair> up;        // [L] t^-1 mod q_i                                        (scale_up)
    std::vector<shoup_pair> one;       // [L] 1 mod q_i                                           (lift)
    // [L]: n_inv[i] gamma t Q_i^-1 mod q_i and w1n[i] gamma t Q_i^-1 mod q_i, the last stage's constants scaled so that the inverse of the Q slabs writes
    // y_i = a_i gamma t Q_i^-1 mod q_i itself, as basis_image::sn, sw do for ModDown
    std::vector<shoup_pair> sn, sw;
    std::vector<shoup_pair> row_t;     // [L] -q_i^-1 gamma^-1 mod t  (= -Q_i D^-1 gamma^-1)      (scale_down)
    std::vector<shoup_pair> row_g;     // [L] -q_i^-1 mod gamma       (= -Q_i D^-1)               (scale_down)
    shoup_pair d_t = {0, 0};           // D mod t
    shoup_pair one_t = {0, 0};         // 1 mod t: its quotient floor(2^64 / t) reduces any 64-bit word modulo t
    shoup_pair g_t = {0, 0};           // gamma^-1 mod t
    uint64_t h = 0;                    // floor(t / 2)
    // agx_ntt_plain_reduce (BGV decryption: the exact centred conversion Q -> t through mixed-radix digits; no inverse modulo t is formed, so any t serves)
    std::vector<uint64_t> q;           // [L] the moduli of Q
    std::vector<shoup_pair> tri;       // [L (L - 1) / 2] q_j^-1 mod q_i at i (i - 1) / 2 + j, j < i: Garner's constants, as ckks_image::tri
    std::vector<shoup_pair> radix_t;   // [L] prod_{k < i} q_k mod t: the weight of digit i modulo t; entry 0 is 1 mod t
};

// Which rule refused a request, the first in this order; nothing is promised about the image then.
enum class plain_fault {
    none,
    source,      // two moduli of Q share a factor (for primes: are equal)
    gamma,       // gamma shares a factor with a modulus of Q (for primes: equals one)
    t_range,     // t < 2 or t >= 2^62: the Shoup products modulo t need 2t < 2^64 and their sums 4t (csrc/bfv_conv_arith.hpp states the bound for its moduli)
    t_source,    // t and some q_i share a factor (for a prime q_i: q_i | t): t has no inverse modulo q_i, D none modulo t
    t_gamma,     // t and gamma share a factor (for a prime gamma: gamma | t)
};
plain_fault prepare_plain_image(plain_image& img, const plain_request& rq);

// Garner's constants of the moduli q[0 .. L), every one odd and > 1: the pair of q_j^-1 mod q_i at i (i - 1) / 2 + j for j < i (L (L - 1) / 2 pairs; a prefix
// serves a prefix of the moduli).  false: two moduli share a factor; nothing is promised about the table then.
bool garner_table(std::vector<shoup_pair>& tri, const uint64_t* q, uint32_t L);

// agx_ntt_ckks_twiddle: tw(len, j) = (cos theta, sin theta), theta = 2 pi (5^j mod 4 len) / (4 len), for len a power of two in [2, 16384] and j < len / 2
// (false otherwise, out untouched).  The angle is reduced exactly in integers to [0, pi / 4] (quadrant, then the complement within it), cosine and sine
// are taken in long double (64-bit significand) and rounded once to double: each component within 2^-53 of the real value.
bool ckks_twiddle(uint32_t len, uint32_t j, double out[2]);

// Everything a CKKS boundary (agx_ntt_ckks_*) keeps on the device, built once on the host (csrc/ckks_arith.hpp has the formulas), for the moduli q[0 .. L),
// every one odd, > 1 and < 2^62, and the ring size n (a power of two, 2 <= n <= 32768):
struct ckks_image {
    std::vector<uint64_t> q;           // [L]
    std::vector<shoup_pair> tri;       // [L (L - 1) / 2] q_j^-1 mod q_i at i (i - 1) / 2 + j, j < i: Garner's constants; a prefix serves a prefix of the moduli
    std::vector<shoup_pair> pow2;      // [L][1024] 2^e mod q_i: the residues of a double from 2^63 on; entry 0 (the constant 1) serves every smaller one
    std::vector<double> tw;            // [n / 2][2] tw(len, j) at len / 2 + j for len = 2 ... n / 2; entry 0 is (1, 0) and is never read
};
// false: two moduli share a factor (for primes: are equal); nothing is promised about the image then
bool prepare_ckks_image(ckks_image& img, const uint64_t* q, uint32_t L, uint32_t n);

// Everything a batching handle (agx_ntt_batch_*) derives from (n, t), built once on the host, for n a plan size (a power of two >= 2: the caller's check) and a prime t = 1 (mod 2n) below 2^62.
// With M = 2n and the exponents e_j = 5^j mod M for j < n / 2, e_{n/2+j} = M - e_j: slot j is the value of the plaintext at psi^{e_j}, which a forward
// transform in the library's order (out[brev(k)] = x(psi^{2k+1})) leaves at word pos(j) = brev((e_j - 1) / 2).  The e_j are the n odd residues modulo M, each
// once, so both tables are permutations of [0, n).
struct batch_image {
    uint64_t psi = 0;                      // the least primitive 2n-th root of unity modulo t
    shoup_pair one_t = {0, 0};             // 1 mod t: its quotient floor(2^64 / t) reduces any 64-bit word modulo t
    std::vector<uint32_t> slot_to_word;    // [n] pos(j)
    std::vector<uint32_t> word_to_slot;    // [n] its inverse
};
enum class batch_fault {
    none,
    modulus,     // t >= 2^62, t != 1 (mod 2n), or t composite
    root,        // no primitive 2n-th root was found (min_primitive_root_2n's search bound)
};
batch_fault prepare_batch_image(batch_image& img, uint32_t n, uint64_t t);

}  // namespace agx
