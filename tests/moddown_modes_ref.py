"""The Python-integer reference model of agx_ntt_basis_mod_down_mode and of a plaintext modulus t (agx_ntt_basis_create_plain,
agx_ntt_keyswitch_create_plain), on top of rns_ref.py.  Per coefficient, with a_j and p_i the coefficient forms of the target and source slabs,
D = prod of the sources, D_i = D / q_i, h = floor(D / 2) under ROUND and 0 under FLOOR, t >= 1 invertible modulo every source:

    y_i   = ((p_i t^-1 mod q_i) + (h mod q_i)) D_i^-1 mod q_i        in [0, q_i)
    V     = sum_i y_i D_i                                             (an integer, 0 <= V < S D)
    out_j = (a_j - (t mod q_j) ((V - h) mod q_j)) D^-1 mod q_j        fully reduced

delta = t (V - h) is congruent to the sources' value modulo D and to 0 modulo t.  The GPU tests are judged against this module; this module is judged
on the CPU by tests/test_moddown_modes_reference.py.  It imports numpy, gpu_util and rns_ref only."""
import numpy as np

from gpu_util import ntt_pi
from rns_ref import (active_of, convert, decompose_ref, digits_of, inner_ref, lift, oracle_forward_set, oracle_inverse_set, product, residues)

FLOOR, ROUND = 0, 1      # AGX_RESCALE_FLOOR, AGX_RESCALE_ROUND


def half(src, mode):
    """h: floor(D / 2) under ROUND, 0 under FLOOR"""
    return product(src) // 2 if mode == ROUND else 0


def lift_mode(p, src, t, mode):
    """p: [S][count] residues (any words) -> V = sum_i y_i D_i per coefficient (Python integers) with y_i = ((p_i t^-1) + h) D_i^-1 mod q_i: rns_ref.lift
    of the residues (p_i t^-1 + h) mod q_i"""
    p = np.asarray(p, dtype=np.uint64).reshape(len(src), -1)
    h = half(src, mode)
    shifted = np.stack([(((p[i] % np.uint64(q)).astype(object) * pow(int(t), -1, int(q)) + h) % int(q)).astype(np.uint64) for i, q in enumerate(src)])
    return lift(shifted, src)


def delta(p, src, t, mode):
    """t (V - h) per coefficient: what the division subtracts first (Python integers, negative where V < h)"""
    return int(t) * (lift_mode(p, src, t, mode) - half(src, mode))


def mod_down_mode(a, p, src, dst, t, mode):
    """agx_ntt_basis_mod_down_mode in coefficient form: a [T][count], p [S][count] residues (any words) -> [T][count] uint64, fully reduced"""
    a = np.asarray(a, dtype=np.uint64).reshape(len(dst), -1)
    d, D = delta(p, src, t, mode), product(src)
    return np.stack([(((a[j] % np.uint64(q)).astype(object) - d) * pow(D, -1, int(q)) % int(q)).astype(np.uint64) for j, q in enumerate(dst)])


def mod_down_mode_ntt(orc, n, xq, xp, src, dst, t, mode):
    """the call as it sees its operands: xq [T][count], xp [S][count] NTT-form words (any words) -> [T][count] NTT-form, fully reduced"""
    return oracle_forward_set(orc, n, dst, mod_down_mode(oracle_inverse_set(orc, n, dst, xq), oracle_inverse_set(orc, n, src, xp), src, dst, t, mode))


def sources_for_y(y, src, t, mode):
    """the source residues p [S][count] whose y_i are the given ones ([S][count], below q_i): p_i = t (y_i D_i - h) mod q_i"""
    D, h = product(src), half(src, mode)
    y = np.asarray(y, dtype=object).reshape(len(src), -1)
    return np.stack([((int(t) * (y[i] * (D // int(q)) - h)) % int(q)).astype(np.uint64) for i, q in enumerate(src)])


def special_sources(src, t, mode):
    """[S][7] source residues: X mod D = 0, 1, H - 1, H, H + 1, D - 1 with H = floor(D / 2) (whatever the mode), then the sources whose every y_i is
    q_i - 1 under (t, mode): the largest V"""
    D = product(src)
    H = D // 2
    first = residues([x % D for x in (0, 1, H - 1, H, H + 1, D - 1)], src)
    return np.concatenate([first, sources_for_y([[int(q) - 1] for q in src], src, t, mode)], axis=1)


# ---- the key switch with a plaintext modulus ------------------------------------------------------------------------------------------------
def keyswitch_plain_ref(orc, n, moduli, shape, chat, key, batch, t, g=1, mode=FLOOR):
    """agx_ntt_keyswitch_apply (g = 1) and _decompose + _apply_decomposed on a handle of agx_ntt_keyswitch_create_plain: rns_ref's decompose_ref (steps 1
    and 2), rns_ref's inner_ref of the digits read through pi_g with the key (step 3), and mod_down_mode for step 4.
    chat [q_count][batch][n], key [digits][2][A][n] (any words below 4q) -> out [2][q_count][batch][n]"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q, special = active[:q_count], active[q_count:]
    A, D = len(active), len(digits_of(shape))
    ext = decompose_ref(orc, n, moduli, shape, chat).reshape(D, A, batch, n)[..., ntt_pi(n, g)]
    acc = inner_ref(ext, np.asarray(key, dtype=np.uint64).reshape(D, 2, A, 1, n), active).reshape(2, A, batch * n)
    return np.stack([mod_down_mode_ntt(orc, n, acc[o, :q_count], acc[o, q_count:], special, Q, t, mode) for o in range(2)]).reshape(2, q_count, batch, n)


def add_key_noise(orc, n, moduli, shape, key, t, rng):
    """key [digits][2][A][n] (NTT form, reduced) with t e_d added to key_{d,0}, e_d ternary: the key of a BGV key switch"""
    active = active_of(moduli, shape)
    key = np.array(key, dtype=np.uint64).reshape(len(digits_of(shape)), 2, len(active), n)
    for d in range(key.shape[0]):
        e = rng.integers(-1, 2, size=n).astype(object) * int(t)
        ehat = oracle_forward_set(orc, n, active, np.stack([(e % int(q)).astype(np.uint64) for q in active]))
        for j, q in enumerate(active):
            key[d, 0, j] = ((key[d, 0, j].astype(object) + ehat[j].astype(object)) % int(q)).astype(np.uint64)
    return key


def deviation(orc, n, moduli, shape, g, batch, chat, shat, out):
    """out_0 + out_1 s - sigma_g(c) sigma_g(s) per coefficient, CRT-centred modulo Q (Python integers, [batch n]); out [2][q_count][batch][n], shat the NTT
    form of s under the active primes (rns_ref.rotation_key_case)"""
    q_count = shape[0]
    Q = active_of(moduli, shape)[:q_count]
    Qp = product(Q)
    pi = ntt_pi(n, g)
    out = np.asarray(out, dtype=np.uint64).reshape(2, q_count, batch, n)
    chat = np.asarray(chat, dtype=np.uint64).reshape(q_count, batch, n)
    dhat = np.stack([((out[0, j].astype(object) + out[1, j].astype(object) * shat[j].astype(object)
                       - (chat[j] % np.uint64(q))[:, pi].astype(object) * shat[j][pi].astype(object)) % int(q)).astype(np.uint64) for j, q in enumerate(Q)])
    res = oracle_inverse_set(orc, n, Q, dhat)
    X = np.zeros(batch * n, dtype=object)
    for j, q in enumerate(Q):
        X = X + res[j].astype(object) * ((Qp // int(q)) * pow(Qp // int(q), -1, int(q)))
    X = X % Qp
    return np.array([int(x) - Qp if int(x) > Qp // 2 else int(x) for x in X], dtype=object)


def plain_bound(shape, s, t):
    """t p_count (1 + ||s||_1): what the key switch with a noise-free key leaves.  out_0 + out_1 s - c s' = -(delta_0 + delta_1 s) / P with
    delta_o = t V_o in FLOOR mode and 0 <= V_o < p_count P (0 <= u < p_count): |delta_o / P| < t p_count, and the product with s adds its 1-norm.
    A condition derived from the formula, not a measurement (as rns_ref.rotation_bound)"""
    return int(t) * shape[2] * (1 + int(np.abs(s).sum()))


# ---- integer polynomials (no transform): the BGV key switch on the CPU -------------------------------------------------------------------------
def negacyclic(a, b, n, q):
    """a b mod (X^n + 1, q) of two coefficient vectors (Python integers), from the definition"""
    out = [0] * n
    for i in range(n):
        for k in range(n):
            if i + k < n:
                out[i + k] += int(a[i]) * int(b[k])
            else:
                out[i + k - n] -= int(a[i]) * int(b[k])
    return np.array([v % int(q) for v in out], dtype=object)


def keyswitch_coeff(n, moduli, shape, c, key, t, mode):
    """the four steps in COEFFICIENT form on one frame, no transform anywhere: c [q_count][n] residues, key [digits][2][A][n] coefficient-form residues
    -> out [2][q_count][n] uint64"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q, special = active[:q_count], active[q_count:]
    acc = [[np.zeros(n, dtype=object) for _ in active] for _ in range(2)]
    for d, (first, count) in enumerate(digits_of(shape)):
        e = convert(np.asarray(c, dtype=np.uint64)[first:first + count], Q[first:first + count], active)
        for o in range(2):
            for j, q in enumerate(active):
                acc[o][j] = (acc[o][j] + negacyclic(e[j], key[d][o][j], n, q)) % int(q)
    out = []
    for o in range(2):
        w = np.stack([acc[o][j].astype(np.uint64) for j in range(len(active))])
        out.append(mod_down_mode(w[:q_count], w[q_count:], special, Q, t, mode))
    return np.stack(out)
