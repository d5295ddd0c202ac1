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

bool basis_constants(const uint64_t* src, uint32_t S, const uint64_t* dst, uint32_t T, uint64_t* dinv, uint64_t* dinv_p, uint64_t* mat, uint64_t* mat_p) {
    // D_i mod m, one factor at a time: S (S - 1) products per modulus, S <= 16
    auto d_mod = [&](uint32_t i, uint64_t m) {
        uint64_t r = 1 % m;
        for (uint32_t k = 0; k < S; ++k)
            if (k != i) r = mul_mod(r, src[k] % m, m);
        return r;
    };
    for (uint32_t i = 0; i < S; ++i) {
        if (!inv_mod_euclid(d_mod(i, src[i]), src[i], &dinv[i])) return false;
        dinv_p[i] = shoup_quotient(dinv[i], src[i]);
    }
    for (uint32_t j = 0; j < T; ++j)
        for (uint32_t i = 0; i < S; ++i) {
            mat[(std::size_t)j * S + i] = d_mod(i, dst[j]);
            mat_p[(std::size_t)j * S + i] = shoup_quotient(mat[(std::size_t)j * S + i], dst[j]);
        }
    return true;
}

bool moddown_constants(const uint64_t* src, uint32_t S, const uint64_t* dst, uint32_t T, const uint64_t* dinv, const uint64_t* n_inv, const uint64_t* w1n,
                       uint64_t* dall, uint64_t* dall_p, uint64_t* sn, uint64_t* sn_p, uint64_t* sw, uint64_t* sw_p) {
    for (uint32_t i = 0; i < S; ++i) {
        sn[i] = mul_mod(n_inv[i], dinv[i], src[i]);
        sn_p[i] = shoup_quotient(sn[i], src[i]);
        sw[i] = mul_mod(w1n[i], dinv[i], src[i]);
        sw_p[i] = shoup_quotient(sw[i], src[i]);
    }
    bool all = true;
    for (uint32_t j = 0; j < T; ++j) {
        uint64_t d = 1 % dst[j];      // D mod dst[j], one factor at a time
        for (uint32_t k = 0; k < S; ++k) d = mul_mod(d, src[k] % dst[j], dst[j]);
        dall[j] = dall_p[j] = 0;
        if (inv_mod_euclid(d, dst[j], &dall[j])) dall_p[j] = shoup_quotient(dall[j], dst[j]);
        else all = false;
    }
    return all;
}

uint64_t half_product_mod(const uint64_t* src, uint32_t S, uint64_t q) {
    uint64_t d = 1 % q;      // D mod q, one factor at a time
    for (uint32_t k = 0; k < S; ++k) d = mul_mod(d, src[k] % q, q);
    const uint64_t d1 = d ? d - 1 : q - 1;      // (D - 1) mod q
    return mul_mod(d1, (q >> 1) + 1, q);        // q odd: (q + 1) / 2 = 2^-1, formed without q + 1
}

bool moddown_mode_constants(const uint64_t* src, uint32_t S, const uint64_t* dst, uint32_t T, uint64_t t, const uint64_t* dinv, const uint64_t* mat, uint64_t* sn,
                            uint64_t* sn_p, uint64_t* sw, uint64_t* sw_p, uint64_t* dmat, uint64_t* dmat_p, uint64_t* cadd, uint64_t* hq) {
    for (uint32_t i = 0; i < S; ++i) {
        const uint64_t q = src[i];
        uint64_t tinv = 0;
        if (!inv_mod_euclid(t % q, q, &tinv)) return false;
        sn[i] = mul_mod(sn[i], tinv, q);
        sn_p[i] = shoup_quotient(sn[i], q);
        sw[i] = mul_mod(sw[i], tinv, q);
        sw_p[i] = shoup_quotient(sw[i], q);
        cadd[i] = mul_mod(half_product_mod(src, S, q), dinv[i], q);
    }
    for (uint32_t j = 0; j < T; ++j) {
        const uint64_t q = dst[j], tq = t % q;
        for (uint32_t i = 0; i < S; ++i) {
            const std::size_t at = (std::size_t)j * S + i;
            dmat[at] = mul_mod(mat[at], tq, q);
            dmat_p[at] = shoup_quotient(dmat[at], q);
        }
        hq[j] = mul_mod(half_product_mod(src, S, q), tq, q);
    }
    return true;
}

bool aux_basis_constants(const uint64_t* src, uint32_t S, const uint64_t* dst, uint32_t T, uint64_t m, const uint64_t* dinv, const uint64_t* mat, aux_constants* out) {
    // D mod q (skip == S) or D_skip mod q, one factor at a time
    auto d_mod = [&](uint32_t skip, uint64_t q) {
        uint64_t r = 1 % q;
        for (uint32_t k = 0; k < S; ++k)
            if (k != skip) r = mul_mod(r, src[k] % q, q);
        return r;
    };
    auto neg = [](uint64_t v, uint64_t q) { return v ? q - v : 0; };
    aux_constants& c = *out;
    for (auto* v : {&c.row, &c.row_p, &c.mdinv, &c.mdinv_p}) v->assign(S, 0);
    for (auto* v : {&c.corr_exact, &c.corr_exact_p, &c.corr_mont, &c.corr_mont_p}) v->assign(T, 0);
    c.mmat.assign((std::size_t)T * S, 0), c.mmat_p.assign((std::size_t)T * S, 0);
    if (!inv_mod_euclid(d_mod(S, m), m, &c.k_exact)) return false;
    c.k_mont = neg(c.k_exact, m);
    c.k_exact_p = shoup_quotient(c.k_exact, m), c.k_mont_p = shoup_quotient(c.k_mont, m);
    for (uint32_t i = 0; i < S; ++i) {
        c.row[i] = d_mod(i, m), c.row_p[i] = shoup_quotient(c.row[i], m);
        c.mdinv[i] = mul_mod(dinv[i], m % src[i], src[i]), c.mdinv_p[i] = shoup_quotient(c.mdinv[i], src[i]);
    }
    for (uint32_t j = 0; j < T; ++j) {
        const uint64_t q = dst[j];
        uint64_t minv = 0;
        if (!inv_mod_euclid(m % q, q, &minv)) return false;
        c.corr_exact[j] = d_mod(S, q), c.corr_exact_p[j] = shoup_quotient(c.corr_exact[j], q);
        c.corr_mont[j] = neg(mul_mod(c.corr_exact[j], minv, q), q), c.corr_mont_p[j] = shoup_quotient(c.corr_mont[j], q);
        for (uint32_t i = 0; i < S; ++i) {
            const std::size_t at = (std::size_t)j * S + i;
            c.mmat[at] = mul_mod(mat[at], minv, q), c.mmat_p[at] = shoup_quotient(c.mmat[at], q);
        }
    }
    return true;
}

}  // namespace agx
