"""The Python-integer reference model of the RNS calls, stated once: fast base conversion (agx_ntt_basis_extend), ModDown (agx_ntt_basis_mod_down),
the ring inner product (agx_ntt_inner_product, _galois) and the hybrid key switch in one call (agx_ntt_keyswitch_apply) and in two halves
(agx_ntt_keyswitch_decompose + agx_ntt_keyswitch_apply_decomposed), with the CPU oracle's transforms over dense frame sets.  The GPU tests are judged
against this module; this module is judged on the CPU by tests/test_rns_ref.py and tests/test_hoist_reference.py.  It imports numpy and gpu_util only.

Throughout, a frame set is [len(moduli)][count] uint64 (any shape of that size is accepted), slab i under moduli[i]; "any words" are reduced below
q_i before they are used, so words spread over the lazy range [0, 4q) are the same inputs as their residues."""
import numpy as np

from gpu_util import ntt_pi, oracle_tables


# ---- integers ---------------------------------------------------------------------------------------------------------------------------
def product(moduli):
    D = 1
    for q in moduli:
        D *= int(q)
    return D


def lift(p, src):
    """p: [S][count] residues (any words) -> V = sum_i y_i D_i per coefficient (Python integers), y_i = p_i D_i^-1 mod q_i; 0 <= V < S D"""
    p = np.asarray(p, dtype=np.uint64).reshape(len(src), -1)
    D = product(src)
    V = np.zeros(p.shape[1], dtype=object)
    for i, q in enumerate(src):
        Di = D // int(q)
        V = V + ((p[i] % np.uint64(q)).astype(object) * pow(Di, -1, int(q)) % int(q)) * Di
    assert all(0 <= v < len(src) * D for v in (V.min(), V.max()))
    return V


def residues(V, moduli):
    """V: non-negative Python integers, a sequence or an object array -> [len(moduli)][count] uint64"""
    V = np.asarray(V, dtype=object).reshape(-1)
    return np.stack([(V % int(q)).astype(np.uint64) for q in moduli])


def convert(x, src, dst):
    """agx_ntt_basis_extend in coefficient form: x [S][count] (any words) -> [T][count] uint64, out_j = V mod q_j"""
    return residues(lift(x, src), dst)


def mod_down(a, p, src, dst):
    """agx_ntt_basis_mod_down in coefficient form: a [T][count], p [S][count] reduced residues -> [T][count] uint64, out_j = (a_j - V) D^-1 mod q_j"""
    a = np.asarray(a, dtype=np.uint64).reshape(len(dst), -1)
    V, D = lift(p, src), product(src)
    return np.stack([((a[j].astype(object) - V) * pow(D, -1, int(q)) % int(q)).astype(np.uint64) for j, q in enumerate(dst)])


def special_values(src):
    """X per coefficient whose V = X + u D lies on a multiple of D or next to one (X = 0, 1, D - 1), X = D - 1 (every residue q_i - 1), their
    neighbours, and the X whose y_i are all q_i - 1 (the largest V) or a single 1 (V = D_k)"""
    D = product(src)
    out = [0, 1, 2, D - 1, D - 2, D // 2, D // 2 + 1]
    out.append(sum((int(q) - 1) * (D // int(q)) for q in src) % D)
    out += [D // int(q) % D for q in src]
    return out


def spread(rng, x, moduli, axis=0):
    """the same residues spread over [0, 4q), the shape kept; `axis` is the prime axis of x"""
    x = np.asarray(x, dtype=np.uint64)
    shape = [1] * x.ndim
    shape[axis] = len(moduli)
    return x + np.array(moduli, dtype=np.uint64).reshape(shape) * rng.integers(0, 4, size=x.shape, dtype=np.uint64)


def ternary(rng, n, weight=None):
    """n coefficients in {-1, 0, 1}: uniform, or exactly `weight` of them nonzero"""
    s = np.zeros(n, dtype=np.int64)
    if weight is None:
        return rng.integers(-1, 2, size=n)
    s[rng.choice(n, size=weight, replace=False)] = rng.choice([-1, 1], size=weight)
    return s


# ---- the oracle over frame sets -----------------------------------------------------------------------------------------------------------
def oracle_forward_set(orc, n, moduli, x):
    """the oracle's forward of the dense [len(moduli)][...][n] set x (reduced), [len(moduli)][count]"""
    x = np.asarray(x, dtype=np.uint64).reshape(len(moduli), -1)
    out = []
    for i, q in enumerate(moduli):
        q, _, tw, pre = oracle_tables(orc, n, q)
        out.append(orc.forward(np.ascontiguousarray(x[i]), q, tw, pre, n))
    return np.stack(out)


def oracle_inverse_set(orc, n, moduli, xhat):
    """the oracle's inverse of NTT-form words (any words: reduced first), [len(moduli)][count]"""
    xhat = np.asarray(xhat, dtype=np.uint64).reshape(len(moduli), -1)
    out = []
    for i, q in enumerate(moduli):
        q, psi, _, _ = oracle_tables(orc, n, q)
        out.append(orc.inverse(np.ascontiguousarray(xhat[i] % np.uint64(q)), q, orc.make_inv_tables(q, psi, n)[0], n))
    return np.stack(out)


def mod_down_ntt(orc, n, xq, xp, src, dst):
    """agx_ntt_basis_mod_down as the call sees it: xq [T][count], xp [S][count] NTT-form words (any words) -> [T][count] NTT-form, fully reduced"""
    return oracle_forward_set(orc, n, dst, mod_down(oracle_inverse_set(orc, n, dst, xq), oracle_inverse_set(orc, n, src, xp), src, dst))


# ---- the inner product ----------------------------------------------------------------------------------------------------------------------
def inner_ref(a, b, moduli):
    """a [T][P][B][n], b [T][O][P][B or 1][n] (any 64-bit words) -> [O][P][B][n] uint64, from the definition"""
    T, P = a.shape[:2]
    O = b.shape[1]
    out = np.empty((O,) + a.shape[1:], dtype=np.uint64)
    for p, q in enumerate(moduli):
        ap = (a[:, p] % np.uint64(q)).astype(object)
        for o in range(O):
            s = (ap * (b[:, o, p] % np.uint64(q)).astype(object)).sum(axis=0)      # Python integers: exact
            out[o, p] = (s % int(q)).astype(np.uint64)
    return out


# ---- the key switch -----------------------------------------------------------------------------------------------------------------------
# A shape is (q_count, p_first, p_count, alpha) on a plan's moduli.  The four steps of include/agx_ntt.h:
#   1. c_j = INTT_j(chat_j);   2. per digit d, V_d = sum_i y_i D_{d,i} with y_i = c_i D_{d,i}^-1 mod q_i, e_{d,j} = V_d mod q_j for every active j;
#   3. acc_{o,j} = sum_d NTT_j(e_{d,j}) o key_{d,o,j} mod q_j;   4. out_{o,j} = NTT_j((INTT_j(acc_{o,j}) - V) D_P^-1 mod q_j), V the lift of acc_o's special slabs.
# Steps 1 and 2 are convert per digit, step 4 is mod_down; step 3 is written out twice, in keyswitch_ref and in apply_decomposed_ref, so that
# test_g_1_is_the_one_call_reference compares two texts.
def digits_of(shape):
    q_count, _, _, alpha = shape
    return [(first, min(alpha, q_count - first)) for first in range(0, q_count, alpha)]


def active_of(moduli, shape):
    q_count, p_first, p_count, _ = shape
    return tuple(moduli[:q_count]) + tuple(moduli[p_first:p_first + p_count])


def keyswitch_ref(orc, n, moduli, shape, chat, key, batch):
    """chat [q_count][batch][n], key [digits][2][A][n] (any words below 4q) -> out [2][q_count][batch][n] uint64, by the four steps"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q, special = active[:q_count], active[q_count:]
    A, digs = len(active), digits_of(shape)
    key = np.asarray(key, dtype=np.uint64).reshape(len(digs), 2, A, 1, n)
    c = oracle_inverse_set(orc, n, Q, chat)                                                       # step 1
    acc = [[np.zeros(batch * n, dtype=object) for _ in range(A)] for _ in range(2)]
    for d, (first, count) in enumerate(digs):                                                     # step 2
        ehat = oracle_forward_set(orc, n, active, convert(c[first:first + count], Q[first:first + count], active))
        for o in range(2):                                                                        # step 3
            for j, q in enumerate(active):
                k = np.broadcast_to((key[d, o, j] % np.uint64(q)).astype(object), (batch, n)).reshape(-1)
                acc[o][j] = acc[o][j] + ehat[j].astype(object) * k
    out = []
    for o in range(2):                                                                            # step 4
        acchat = np.stack([(acc[o][j] % int(q)).astype(np.uint64) for j, q in enumerate(active)])
        out.append(mod_down_ntt(orc, n, acchat[:q_count], acchat[q_count:], special, Q))
    return np.stack(out).reshape(2, q_count, batch, n)


def decompose_ref(orc, n, moduli, shape, chat):
    """steps 1 and 2: chat [q_count][batch][n] (any words below 4q) -> ext [digits][A][batch n] uint64, fully reduced"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q = active[:q_count]
    c = oracle_inverse_set(orc, n, Q, chat)
    return np.stack([oracle_forward_set(orc, n, active, convert(c[first:first + count], Q[first:first + count], active)) for first, count in digits_of(shape)])


def apply_decomposed_ref(orc, n, moduli, shape, ext, key, batch, g):
    """steps 3 and 4 with ext read through pi_g = ntt_pi(n, g) per frame: ext [digits][A][batch n], key [digits][2][A][n] (any words below 4q) ->
    out [2][q_count][batch][n]"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q, special = active[:q_count], active[q_count:]
    A, D = len(active), len(digits_of(shape))
    key = np.asarray(key, dtype=np.uint64).reshape(D, 2, A, 1, n)
    gathered = np.asarray(ext, dtype=np.uint64).reshape(D, A, batch, n)[..., ntt_pi(n, g)]
    out = []
    for o in range(2):
        acchat = []
        for j, q in enumerate(active):                                                            # step 3
            s = np.zeros((batch, n), dtype=object)
            for d in range(D):
                s = s + gathered[d, j].astype(object) * (key[d, o, j] % np.uint64(q)).astype(object)
            acchat.append((s % int(q)).astype(np.uint64).reshape(-1))
        acchat = np.stack(acchat)
        out.append(mod_down_ntt(orc, n, acchat[:q_count], acchat[q_count:], special, Q))          # step 4
    return np.stack(out).reshape(2, q_count, batch, n)


def hoisted_ref(orc, n, moduli, shape, chat, key, batch, g):
    """keyswitch_ref with each ehat[j] indexed by ntt_pi(n, g) per frame"""
    return apply_decomposed_ref(orc, n, moduli, shape, decompose_ref(orc, n, moduli, shape, chat), key, batch, g)


def rotation_key_case(orc, n, moduli, shape, g, batch, seed):
    """(chat [q_count][batch][n], key [digits][2][A][n], s, shat [A][n]): random chat, a ternary s of Hamming weight 8 and the noise-free key
    key_{d,1} = a_d random, key_{d,0} = -a_d s + D_P G_d sigma_g(s) with G_d = (Q / D_d) [(Q / D_d)^-1 mod D_d], everything in NTT form"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q, A, digs = active[:q_count], len(active), digits_of(shape)
    Qp, DP = product(Q), product(active[q_count:])
    rng = np.random.default_rng(seed)
    s = ternary(rng, n, 8)
    shat = oracle_forward_set(orc, n, active, np.stack([(s % int(q)).astype(np.uint64) for q in active]))
    rotated = shat[:, ntt_pi(n, g)]      # the NTT form of sigma_g(s)
    key = np.empty((len(digs), 2, A, n), dtype=np.uint64)
    for d, (first, count) in enumerate(digs):
        Dd = product(Q[first:first + count])
        G = (Qp // Dd) * pow(Qp // Dd, -1, Dd)
        for j, q in enumerate(active):
            ahat = rng.integers(0, int(q), size=n, dtype=np.uint64)
            key[d, 1, j] = ahat
            key[d, 0, j] = ((DP * G % int(q)) * rotated[j].astype(object) - ahat.astype(object) * shat[j].astype(object)) % int(q)
    chat = np.stack([rng.integers(0, int(q), size=(batch, n), dtype=np.uint64) for q in Q])
    return chat, key, s, shat


def rotation_deviation(orc, n, moduli, shape, g, batch, chat, shat, out):
    """the largest |coefficient| of out_0 + out_1 s - sigma_g(c) sigma_g(s), CRT-centred modulo Q; out [2][q_count][batch][n]"""
    q_count = shape[0]
    Q = active_of(moduli, shape)[:q_count]
    Qp = product(Q)
    pi = ntt_pi(n, g)
    out = np.asarray(out, dtype=np.uint64).reshape(2, q_count, batch, n)
    dhat = np.stack([((out[0, j].astype(object) + out[1, j].astype(object) * shat[j].astype(object)
                       - chat[j][:, pi].astype(object) * shat[j][pi].astype(object)) % int(q)).astype(np.uint64) for j, q in enumerate(Q)])
    res = oracle_inverse_set(orc, n, Q, dhat)
    X = np.zeros(batch * n, dtype=object)
    for j, q in enumerate(Q):
        X = X + res[j].astype(object) * ((Qp // int(q)) * pow(Qp // int(q), -1, int(q)))
    X = X % Qp
    return max(abs(int(x) - Qp if int(x) > Qp // 2 else int(x)) for x in X)


def rotation_bound(shape, s):
    """p_count (1 + ||s||_1): what the two approximate conversions leave, a condition and not a measurement (test_it_switches_keys)"""
    return shape[2] * (1 + int(np.abs(s).sum()))


# ---- frames too many for the host -------------------------------------------------------------------------------------------------------------
def device_residues(torch, dev, moduli, batch, n, seed, bound=None):
    """[len(moduli)][batch][n] on the device, slab i uniform below moduli[i] (or below `bound`): any such words are NTT-form frames"""
    g = torch.Generator(device=dev.device)
    g.manual_seed(seed)
    d = dev.empty(len(moduli) * batch * n)
    v = d.view(len(moduli), -1)
    for i, q in enumerate(moduli):
        v[i] = torch.randint(0, int(q if bound is None else bound), (batch * n,), generator=g, device=dev.device, dtype=torch.int64)
    return d
