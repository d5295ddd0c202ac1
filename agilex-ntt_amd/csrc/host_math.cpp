#include "host_math.hpp"

namespace agx {

typedef unsigned __int128 u128;

uint64_t mul_mod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((u128)a * b % q); }

uint64_t pow_mod(uint64_t a, uint64_t e, uint64_t q) {
    uint64_t r = 1 % q, base = a % q;
    for (; e; e >>= 1) {
        if (e & 1) r = mul_mod(r, base, q);
        base = mul_mod(base, base, q);
    }
    return r;
}

uint64_t inv_mod(uint64_t a, uint64_t q) { return pow_mod(a, q - 2, q); }

// Miller-Rabin with the first twelve primes as witnesses: deterministic below 3.3e24
bool is_prime_u64(uint64_t q) {
    if (q < 2) return false;
    const uint64_t wit[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
    for (uint64_t p : wit)
        if (q % p == 0) return q == p;
    uint64_t odd = q - 1;
    int twos = 0;
    while ((odd & 1) == 0) { odd >>= 1; ++twos; }
    for (uint64_t a : wit) {
        uint64_t y = pow_mod(a, odd, q);
        if (y == 1 || y == q - 1) continue;
        bool witness = true;
        for (int k = 1; k < twos && witness; ++k) {
            y = mul_mod(y, y, q);
            if (y == q - 1) witness = false;
        }
        if (witness) return false;
    }
    return true;
}

std::vector<uint64_t> find_ntt_primes(uint32_t bits, uint32_t n, uint32_t count) {
    std::vector<uint64_t> found;
    if (bits < 2 || bits > 62 || !is_pow2(n)) return found;
    const uint64_t two_n = 2ull * n;
    const uint64_t limit = (1ull << bits) - 1;
    if (limit <= two_n) return found;
    uint64_t cand = limit - ((limit - 1) % two_n);  // largest value <= limit that is 1 mod 2n
    while (found.size() < count && cand > two_n) {
        if (is_prime_u64(cand)) found.push_back(cand);
        cand -= two_n;
    }
    return found;
}

bool is_primitive_root_2n(uint64_t psi, uint64_t q, uint32_t n) {
    // the multiplicative order divides 2n (a power of two) and is exactly 2n iff psi^n = -1
    return psi > 1 && psi < q && pow_mod(psi, n, q) == q - 1;
}

uint64_t min_primitive_root_2n(uint64_t q, uint32_t n) {
    const uint64_t two_n = 2ull * n;
    if (q < 3 || (q - 1) % two_n) return 0;
    const uint64_t cofactor = (q - 1) / two_n;
    uint64_t some_root = 0;
    for (uint64_t g = 2; g < q && g < 100000; ++g) {
        uint64_t r = pow_mod(g, cofactor, q);
        if (is_primitive_root_2n(r, q, n)) { some_root = r; break; }
    }
    if (!some_root) return 0;
    // the primitive 2n-th roots are exactly the odd powers of any one of them
    const uint64_t sq = mul_mod(some_root, some_root, q);
    uint64_t least = some_root, walk = some_root;
    for (uint32_t k = 1; k < n; ++k) {
        walk = mul_mod(walk, sq, q);
        if (walk < least) least = walk;
    }
    return least;
}

bool inv_mod_euclid(uint64_t a, uint64_t q, uint64_t* inv) {
    // extended Euclid on (a mod q, q) with the coefficient of a kept mod q; gcd 1 <=> invertible
    __int128 r0 = q, r1 = a % q, t0 = 0, t1 = 1;
    while (r1 != 0) {
        const __int128 k = r0 / r1, r2 = r0 - k * r1, t2 = t0 - k * t1;
        r0 = r1, r1 = r2, t0 = t1, t1 = t2;
    }
    if (r0 != 1) return false;
    *inv = (uint64_t)(t0 < 0 ? t0 + (__int128)q : t0);
    return true;
}

uint64_t shoup_quotient(uint64_t w, uint64_t q) { return (uint64_t)(((u128)w << 64) / q); }

fold_twiddle fold_twiddle_pack(uint64_t w, uint64_t q) {
    const uint64_t low29 = (1ull << 29) - 1, wc = mul_mod(w, 1ull << 32, q);
    return {(w & low29) | (w >> 29) << 32, (wc & low29) | (wc >> 29) << 32};
}

void power_tables_bitrev(uint64_t q, uint64_t base, uint32_t n, uint64_t* tw, uint64_t* pre) {
    const int lg = log2u(n);
    std::vector<uint64_t> pw(n);
    pw[0] = 1 % q;
    for (uint32_t i = 1; i < n; ++i) pw[i] = mul_mod(pw[i - 1], base, q);
    for (uint32_t j = 0; j < n; ++j) {
        tw[j] = pw[bit_reverse(j, lg)];
        pre[j] = shoup_quotient(tw[j], q);
    }
}

// D mod q (skip == S) or D_skip mod q, one factor at a time: at most S products per call, S <= 16
static uint64_t product_mod(const uint64_t* src, uint32_t S, uint32_t skip, uint64_t q) {
    uint64_t r = 1 % q;
    for (uint32_t k = 0; k < S; ++k)
        if (k != skip) r = mul_mod(r, src[k] % q, q);
    return r;
}

uint64_t half_product_mod(uint64_t d_mod_q, uint64_t q) {
    const uint64_t d1 = d_mod_q ? d_mod_q - 1 : q - 1;      // (D - 1) mod q
    return mul_mod(d1, (q >> 1) + 1, q);                     // q odd: (q + 1) / 2 = 2^-1, formed without q + 1
}
uint64_t half_product_mod(const uint64_t* src, uint32_t S, uint64_t q) { return half_product_mod(product_mod(src, S, S, q), q); }

basis_fault prepare_basis_image(basis_image& img, const basis_request& rq) {
    const uint32_t S = rq.S, T = rq.T;
    const uint64_t m = rq.m;
    auto neg = [](uint64_t v, uint64_t q) { return v ? q - v : 0; };
    img = basis_image{};
    for (uint32_t i = 0; i < S; ++i) {
        const uint64_t q = rq.src[i];
        uint64_t dinv = 0;
        if (!inv_mod_euclid(product_mod(rq.src, S, i, q), q, &dinv)) return basis_fault::source;
        img.dinv.push_back(shoup_pair::of(dinv, q));
    }
    for (uint32_t i = 0; i < S; ++i) {
        const uint64_t q = rq.src[i], dinv = img.dinv[i].w;
        uint64_t tinv = 0;
        if (!inv_mod_euclid(rq.t % q, q, &tinv)) return basis_fault::t;
        const uint64_t scale = mul_mod(dinv, tinv, q);      // t^-1 D_i^-1
        img.sn.push_back(shoup_pair::of(mul_mod(rq.n_inv[i], scale, q), q));
        img.sw.push_back(shoup_pair::of(mul_mod(rq.w1n[i], scale, q), q));
        img.round_src.push_back({mul_mod(half_product_mod(product_mod(rq.src, S, S, q), q), dinv, q), q});
    }
    uint64_t k = 0;
    if (m) {
        if (!inv_mod_euclid(product_mod(rq.src, S, S, m), m, &k)) return basis_fault::aux;
        img.k_exact = shoup_pair::of(k, m), img.k_mont = shoup_pair::of(neg(k, m), m);
        for (uint32_t i = 0; i < S; ++i) {
            const uint64_t q = rq.src[i];
            img.aux_row.push_back(shoup_pair::of(product_mod(rq.src, S, i, m), m));
            img.aux_mdinv.push_back(shoup_pair::of(mul_mod(img.dinv[i].w, m % q, q), q));
        }
    }
    img.moddown_legal = true;
    for (uint32_t j = 0; j < T; ++j) {
        const uint64_t q = rq.dst[j], tq = rq.t % q, d = product_mod(rq.src, S, S, q);
        uint64_t dall = 0, minv = 0;
        if (inv_mod_euclid(d, q, &dall)) img.dall.push_back(shoup_pair::of(dall, q));
        else img.dall.push_back({0, 0}), img.moddown_legal = false;
        img.round_dst.push_back(mul_mod(half_product_mod(d, q), tq, q));
        if (m) {
            if (!inv_mod_euclid(m % q, q, &minv)) return basis_fault::aux;
            img.aux_corr_exact.push_back(shoup_pair::of(d, q));
            img.aux_corr_mont.push_back(shoup_pair::of(neg(mul_mod(d, minv, q), q), q));
        }
        for (uint32_t i = 0; i < S; ++i) {
            const uint64_t di = product_mod(rq.src, S, i, q);
            img.mat.push_back(shoup_pair::of(di, q));
            img.down_mat.push_back(shoup_pair::of(mul_mod(di, tq, q), q));
            if (m) img.aux_mmat.push_back(shoup_pair::of(mul_mod(di, minv, q), q));
        }
    }
    if (!m || !rq.quot_t) return basis_fault::none;
    // the quotient: E = prod dst[j]
    for (uint32_t j = 0; j < T; ++j) {
        const uint64_t q = rq.dst[j];
        uint64_t ejinv = 0;
        if (!inv_mod_euclid(product_mod(rq.dst, T, j, q), q, &ejinv)) return basis_fault::quotient;
        const uint64_t scale = mul_mod(ejinv, rq.quot_t % q, q);      // t E_j^-1
        img.quot_dn.push_back(shoup_pair::of(mul_mod(rq.dst_n_inv[j], scale, q), q));
        img.quot_dw.push_back(shoup_pair::of(mul_mod(rq.dst_w1n[j], scale, q), q));
    }
    for (uint32_t i = 0; i <= S; ++i) {
        const uint64_t q = i < S ? rq.src[i] : m;
        uint64_t einv = 0;
        if (!inv_mod_euclid(product_mod(rq.dst, T, T, q), q, &einv)) return basis_fault::quotient;
        const uint64_t scale = mul_mod(mul_mod(einv, rq.quot_t % q, q), i < S ? img.dinv[i].w : 1 % q, q);      // t E^-1 D_i^-1; for m: t E^-1
        img.quot_sn.push_back(shoup_pair::of(mul_mod(i < S ? rq.n_inv[i] : rq.aux_n_inv, scale, q), q));
        img.quot_sw.push_back(shoup_pair::of(mul_mod(i < S ? rq.w1n[i] : rq.aux_w1n, scale, q), q));
    }
    for (uint32_t j = 0; j < T; ++j)
        for (uint32_t i = 0; i <= S; ++i) {
            const uint64_t q = i < S ? rq.src[i] : m;
            uint64_t qjinv = 0;
            if (!inv_mod_euclid(rq.dst[j] % q, q, &qjinv)) return basis_fault::quotient;
            img.quot_mat.push_back(shoup_pair::of(mul_mod(qjinv, i < S ? img.dinv[i].w : 1 % q, q), q));
        }
    return basis_fault::none;
}

plain_fault prepare_plain_image(plain_image& img, const plain_request& rq) {
    const uint32_t L = rq.L;
    const uint64_t t = rq.t, gamma = rq.gamma;
    auto neg = [](uint64_t v, uint64_t q) { return v ? q - v : 0; };
    img = plain_image{};
    std::vector<uint64_t> qinv(L);      // Q_i^-1 mod q_i
    for (uint32_t i = 0; i < L; ++i)
        if (!inv_mod_euclid(product_mod(rq.q, L, i, rq.q[i]), rq.q[i], &qinv[i])) return plain_fault::source;
    for (uint32_t i = 0; i < L; ++i) {
        uint64_t w = 0;
        if (!inv_mod_euclid(rq.q[i] % gamma, gamma, &w)) return plain_fault::gamma;
        img.row_g.push_back(shoup_pair::of(neg(w, gamma), gamma));
    }
    if (t < 2 || t >= (1ull << 62)) return plain_fault::t_range;
    for (uint32_t i = 0; i < L; ++i) {
        const uint64_t q = rq.q[i];
        uint64_t tinv = 0;
        if (!inv_mod_euclid(t % q, q, &tinv)) return plain_fault::t_source;
        const uint64_t scale = mul_mod(mul_mod(gamma % q, t % q, q), qinv[i], q);      // gamma t Q_i^-1
        img.up.push_back(shoup_pair::of(tinv, q));
        img.one.push_back(shoup_pair::of(1, q));
        img.sn.push_back(shoup_pair::of(mul_mod(rq.n_inv[i], scale, q), q));
        img.sw.push_back(shoup_pair::of(mul_mod(rq.w1n[i], scale, q), q));
    }
    uint64_t g = 0;
    if (!inv_mod_euclid(gamma % t, t, &g)) return plain_fault::t_gamma;
    for (uint32_t i = 0; i < L; ++i) {
        uint64_t w = 0;
        if (!inv_mod_euclid(rq.q[i] % t, t, &w)) return plain_fault::t_source;      // gcd(q_i, t) = 1 was found above: not reached
        img.row_t.push_back(shoup_pair::of(neg(mul_mod(w, g, t), t), t));
    }
    img.d_t = shoup_pair::of(product_mod(rq.q, L, L, t), t);
    img.one_t = shoup_pair::of(1, t);
    img.g_t = shoup_pair::of(g, t);
    img.h = t >> 1;
    img.q.assign(rq.q, rq.q + L);
    if (!garner_table(img.tri, rq.q, L)) return plain_fault::source;      // the moduli were found coprime above: not reached
    for (uint32_t i = 0; i < L; ++i) img.radix_t.push_back(shoup_pair::of(product_mod(rq.q, i, i, t), t));
    return plain_fault::none;
}

bool garner_table(std::vector<shoup_pair>& tri, const uint64_t* q, uint32_t L) {
    tri.clear();
    for (uint32_t i = 1; i < L; ++i)
        for (uint32_t j = 0; j < i; ++j) {
            uint64_t w = 0;
            if (!inv_mod_euclid(q[j] % q[i], q[i], &w)) return false;
            tri.push_back(shoup_pair::of(w, q[i]));
        }
    return true;
}

bool ckks_twiddle(uint32_t len, uint32_t j, double out[2]) {
    if (len < 2 || len > 16384 || (len & (len - 1)) || j >= len / 2) return false;
    const uint32_t m = 4 * len, quarter = len;                 // theta = 2 pi r / m, m >= 8
    const uint32_t r = (uint32_t)pow_mod(5, j, m);             // odd
    const uint32_t quadrant = r / quarter, in = r % quarter;   // theta = quadrant pi / 2 + 2 pi in / m
    const bool swap = in > quarter / 2;                        // the complement pi / 2 - phi: cosine and sine change places
    const uint32_t rr = swap ? quarter - in : in;              // 2 pi rr / m in [0, pi / 4]
    const long double pi = 3.141592653589793238462643383279502884L;
    const long double phi = (2.0L * pi * (long double)rr) / (long double)m;
    long double c = __builtin_cosl(phi), s = __builtin_sinl(phi);
    if (swap) { const long double t = c; c = s, s = t; }
    switch (quadrant) {
        case 0: out[0] = (double)c, out[1] = (double)s; break;
        case 1: out[0] = (double)-s, out[1] = (double)c; break;
        case 2: out[0] = (double)-c, out[1] = (double)-s; break;
        default: out[0] = (double)s, out[1] = (double)-c; break;
    }
    return true;
}

bool prepare_ckks_image(ckks_image& img, const uint64_t* q, uint32_t L, uint32_t n) {
    img = ckks_image{};
    img.q.assign(q, q + L);
    if (!garner_table(img.tri, q, L)) return false;
    for (uint32_t i = 0; i < L; ++i) {
        uint64_t w = 1 % q[i];
        for (uint32_t e = 0; e < 1024; ++e) {
            img.pow2.push_back(shoup_pair::of(w, q[i]));
            w = (w << 1) >= q[i] ? (w << 1) - q[i] : w << 1;
        }
    }
    const uint32_t half = n / 2 ? n / 2 : 1;
    img.tw.assign(2 * (size_t)half, 0.0);
    img.tw[0] = 1.0;
    for (uint32_t len = 2; len <= n / 2; len <<= 1)
        for (uint32_t j = 0; j < len / 2; ++j) ckks_twiddle(len, j, &img.tw[2 * (size_t)(len / 2 + j)]);
    return true;
}

batch_fault prepare_batch_image(batch_image& img, uint32_t n, uint64_t t) {
    img = batch_image{};
    const uint64_t M = 2ull * n;
    if (t >= (1ull << 62) || t < 3 || (t - 1) % M || !is_prime_u64(t)) return batch_fault::modulus;
    img.psi = min_primitive_root_2n(t, n);
    if (!img.psi) return batch_fault::root;
    img.one_t = shoup_pair::of(1, t);
    const int lg = log2u(n);
    img.slot_to_word.assign(n, 0), img.word_to_slot.assign(n, 0);
    uint64_t e = 1;
    for (uint32_t j = 0; j < n / 2; ++j) {
        const uint32_t lo = bit_reverse((uint32_t)((e - 1) / 2), lg), hi = bit_reverse((uint32_t)((M - e - 1) / 2), lg);
        img.slot_to_word[j] = lo, img.slot_to_word[n / 2 + j] = hi;
        img.word_to_slot[lo] = j, img.word_to_slot[hi] = n / 2 + j;
        e = e * 5 % M;
    }
    return batch_fault::none;
}

}  // namespace agx
