// plain_arith.hpp -- the per-word steps of agx_ntt_plain_scale_up, _lift and _scale_down (BFV's plaintext boundary: the scaling of a plaintext modulo t into
// Q, its centred lift, and the rounding of decryption through one auxiliary prime gamma; BEHZ, Bajard et al., SAC 2016, section 3), beside those of
// bfv_conv_arith.hpp and bfv_quotient_arith.hpp, which it uses and does not restate.  Compiles for the device (plain_kernels.hpp) and for the host
// (tests/plain_selftest.cpp runs this same text against unsigned __int128), as bfv_quotient_arith.hpp does: no HIP header is needed on the host.
//
// With D = prod q_i over the L primes of Q, Q_i = D / q_i, h = floor(t / 2), 2 <= t < 2^62 (ANY such t: even, a power of two, composite, above every q_i):
//   scale_up    m' = m mod t,  rho = ((D mod t) m' + h) mod t,  U = (D m' + h - rho) / t = floor((2 D m' + t) / (2t)),  out_i = (h - rho) t^-1 mod q_i
//               since D = 0 (mod q_i): one product modulo t per coefficient, one signed Shoup product per prime.
//   lift        out_i = m' mod q_i for m' < ceil(t / 2) = t - h, (m' - t) mod q_i from there on: the same signed product with the constant 1.
//   scale_down  the scaled inverse hands the kernel y_i = a_i gamma t Q_i^-1 mod q_i in [0, q_i); with V = sum_i y_i Q_i and Q_i D^-1 = q_i^-1,
//               s_t g = sum_i y_i (-q_i^-1 gamma^-1 mod t)  mod t   (g = gamma^-1 mod t is folded into the row: s_t g is what the last line needs),
//               s_gamma = sum_i y_i (-q_i^-1 mod gamma)  mod gamma,   c = centre_gamma(s_gamma),   m = s_t g - c g  mod t.
// Ranges.  A Shoup product w y - floor(w' y / 2^64) q lies in [0, 2q) for ANY 64-bit y, any w < q and any modulus q with 2q < 2^64, odd or even
// (bfv_conv_arith.hpp): that is what lets a word of one modulus meet a constant of another, and what asks for t < 2^62 (quot_accumulate forms 4t).
//   plain_reduce    any 64-bit m -> m mod t in [0, t): bfv_shoup by the constant 1 (1 < t), whose quotient is floor(2^64 / t) < 2^63.
//   plain_scaled    mp in [0, t): rho = ((D mod t) mp + h) mod t in [0, t) -- the product in [0, t), the sum below 2t < 2^63 -- and the signed value
//                   h - rho as a magnitude below t and a sign (0 is positive): *negative = rho > h.
//   plain_centred   mp in [0, t): mp for mp < t - h, mp - t (magnitude t - mp in [1, h]) from there on; for t = 2: 0 -> 0, 1 -> -1.
//   plain_residue   a signed value (mag < 2^62: a residue of ANOTHER modulus, it may exceed q) times a constant c < q, modulo q, fully reduced: bfv_correct
//                   on an empty sum computes 0 - alpha c, so alpha = -(the value): the sign is handed over flipped.  -0 = 0 either way.
//   plain_round     acc_t in [0, 2t) and acc_g in [0, 2 gamma) as quot_accumulate leaves them, gamma odd: acc_g is brought below gamma and centred
//                   (|c| <= (gamma - 1) / 2 < 2^61, both edges as bfv_centre has them), then bfv_correct with the constant g: acc_t - c g mod t in [0, t).
//   plain_from_digits   agx_ntt_plain_reduce (BGV decryption), after ckks_arith.hpp's Garner digits v_i in [0, q_i) of X mod D and its sign test: with the row
//                   r_i = prod_{k < i} q_k mod t, X mod D = sum_i v_i prod_{k < i} q_k and the centred X is that, less D when negative, so
//                   m = f ((sum_i v_i r_i) - [negative] (D mod t)) mod t.  quot_accumulate keeps the sum in [0, 2t) for ANY 64-bit v_i (a digit may exceed t);
//                   one subtraction brings it below t, one more takes D mod t off, and ONE Shoup product by f = factor mod t gives [0, t).  No inverse
//                   modulo t appears: an even t, a power of two and t = 2 serve as any other.
#pragma once
#include "bfv_quotient_arith.hpp"
#include "ckks_arith.hpp"

namespace agx {

AGX_HD uint64_t plain_reduce(uint64_t m, uint64_t one_p, uint64_t t) { return bfv_shoup(m, 1, one_p, t); }

AGX_HD uint64_t plain_scaled(uint64_t mp, uint64_t d, uint64_t dp, uint64_t h, uint64_t t, bool* negative) {
    const uint64_t s = bfv_shoup(mp, d, dp, t) + h, rho = s >= t ? s - t : s;
    *negative = rho > h;
    return *negative ? rho - h : h - rho;
}

AGX_HD uint64_t plain_centred(uint64_t mp, uint64_t h, uint64_t t, bool* negative) {
    *negative = mp >= t - h;
    return *negative ? t - mp : mp;
}

AGX_HD uint64_t plain_residue(uint64_t mag, bool negative, uint64_t c, uint64_t cp, uint64_t q) { return bfv_correct(0, mag, !negative, c, cp, q); }

AGX_HD uint64_t plain_round(uint64_t acc_t, uint64_t acc_g, uint64_t gamma, uint64_t g, uint64_t gp, uint64_t t) {
    bool negative;
    const uint64_t mag = bfv_centre(acc_g >= gamma ? acc_g - gamma : acc_g, gamma, &negative);
    return bfv_correct(acc_t, mag, negative, g, gp, t);
}

// row: the pairs {r_i, quotient}, two words each (the host has no ulonglong2)
template <int SMAX>
AGX_HD uint64_t plain_from_digits(const uint64_t (&v)[SMAX], bool negative, uint32_t L, const uint64_t* row, uint64_t t, uint64_t d, uint64_t f, uint64_t fp) {
    const uint64_t t2 = t << 1;
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < SMAX; ++i)
        if ((uint32_t)i < L) acc = quot_accumulate(acc, v[i], row[2 * i], row[2 * i + 1], t, t2);
    uint64_t a = acc >= t ? acc - t : acc;
    if (negative) a = a - d + (a < d ? t : 0);
    return bfv_shoup(a, f, fp, t);
}

}  // namespace agx
