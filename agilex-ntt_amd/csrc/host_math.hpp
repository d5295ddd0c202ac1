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

// The constants of a fast RNS base conversion (agx_ntt_basis_extend) from the moduli src[0 .. S) to the moduli dst[0 .. T), every modulus
// odd, > 1 and < 2^62.  With D = prod src[i] and D_i = D / src[i]:
//   dinv[i] = D_i^-1 mod src[i],   mat[j * S + i] = D_i mod dst[j],   dinv_p / mat_p their precomputed quotients (shoup_quotient).
// false, nothing promised about the outputs, when some D_i is not invertible modulo src[i]: two source moduli share a factor (for primes:
// are equal).  A target that is itself source k gets D_i mod dst[j] = 0 for i != k, so the conversion hands that residue through.
bool basis_constants(const uint64_t* src, uint32_t S, const uint64_t* dst, uint32_t T, uint64_t* dinv, uint64_t* dinv_p, uint64_t* mat, uint64_t* mat_p);

// What agx_ntt_basis_mod_down needs beyond basis_constants, for the same moduli (dinv as basis_constants wrote it):
//   dall[j] = D^-1 mod dst[j] with its quotient dall_p[j] -- {0, 0} where D is not invertible modulo dst[j] (dst[j] shares a factor with a source;
//     for primes: equals one); the return value says whether every one exists;
//   sn[i] = n_inv[i] dinv[i] mod src[i] and sw[i] = w1n[i] dinv[i] mod src[i] with their quotients sn_p / sw_p: the two constants of an inverse
//     transform's last stage (n^-1 mod src[i] and inv_twiddle[1] n^-1 mod src[i], both below src[i]) scaled by D_i^-1, so that the inverse of
//     the source slabs writes y_i = p_i D_i^-1 mod src[i] itself.
bool moddown_constants(const uint64_t* src, uint32_t S, const uint64_t* dst, uint32_t T, const uint64_t* dinv, const uint64_t* n_inv, const uint64_t* w1n,
                       uint64_t* dall, uint64_t* dall_p, uint64_t* sn, uint64_t* sn_p, uint64_t* sw, uint64_t* sw_p);

// h mod q for h = floor(D / 2), D = prod src[i] odd, q odd and > 1: h is a multi-word integer (S up to 16 moduli of 62 bits) and is never formed.
// 2 h = D - 1 exactly, so h = (D - 1) 2^-1 (mod q) with 2^-1 = (q + 1) / 2; D mod q is taken one factor at a time in 128 bits.
uint64_t half_product_mod(const uint64_t* src, uint32_t S, uint64_t q);

// What agx_ntt_basis_mod_down_mode and a plaintext modulus t >= 1 (agx_ntt_basis_create_plain) need beyond the two sets above, for the same moduli
// (dinv, mat as basis_constants wrote them; sn, sw as moddown_constants wrote them).  t is any 64-bit value, reduced per modulus here.
//   sn[i], sw[i] are multiplied by t^-1 mod src[i] in place (quotients sn_p / sw_p again): the scaled inverse then writes p_i t^-1 D_i^-1 mod src[i];
//   dmat[j * S + i] = t D_i mod dst[j] with its quotient dmat_p: ModDown's matrix, a copy of its own (agx_ntt_basis_extend keeps mat);
//   cadd[i] = h D_i^-1 mod src[i] and hq[j] = t h mod dst[j], h = floor(D / 2): the two constants of AGX_RESCALE_ROUND (csrc/moddown_arith.hpp).
// false, nothing promised about the outputs, when t has no inverse modulo some source (for prime sources: t = 0 modulo one of them).
// With t = 1 nothing changes: sn, sw stay, dmat = mat.
bool moddown_mode_constants(const uint64_t* src, uint32_t S, const uint64_t* dst, uint32_t T, uint64_t t, const uint64_t* dinv, const uint64_t* mat, uint64_t* sn,
                            uint64_t* sn_p, uint64_t* sw, uint64_t* sw_p, uint64_t* dmat, uint64_t* dmat_p, uint64_t* cadd, uint64_t* hq);

// What agx_ntt_basis_extend_exact and agx_ntt_basis_extend_mont need beyond basis_constants (dinv, mat as it wrote them), for the same moduli and an
// auxiliary modulus m, odd, > 1 and < 2^62 (csrc/bfv_conv_arith.hpp has the formulas); every word comes with its quotient (_p):
//   row[i] = D_i mod m;   k_exact = D^-1 mod m,   k_mont = -D^-1 mod m;
//   corr_exact[j] = D mod dst[j];
//   mdinv[i] = m dinv[i] mod src[i],   mmat[j * S + i] = mat[j * S + i] m^-1 mod dst[j],   corr_mont[j] = -D m^-1 mod dst[j].
// false, nothing promised about the outputs, when D has no inverse modulo m or m none modulo some target (for primes: m equals a source or a target).
struct aux_constants {
    std::vector<uint64_t> row, row_p, corr_exact, corr_exact_p, mdinv, mdinv_p, mmat, mmat_p, corr_mont, corr_mont_p;
    uint64_t k_exact = 0, k_exact_p = 0, k_mont = 0, k_mont_p = 0;
};
bool aux_basis_constants(const uint64_t* src, uint32_t S, const uint64_t* dst, uint32_t T, uint64_t m, const uint64_t* dinv, const uint64_t* mat, aux_constants* out);

}  // namespace agx
