"""The Python-integer reference of the double-hoisted linear transform, on top of rns_ref.py: agx_ntt_keyswitch_accumulate_decomposed (the inner-product
half of apply_decomposed with a weight and an accumulate), agx_ntt_mul_add_galois, and their composition with ModDown (agx_ntt_keyswitch_mod_down is
rns_ref.mod_down_ntt on each half of acc).  Judged on the CPU by tests/test_dhoist_reference.py; the GPU tests are judged against it.

A weight is [A][weight_batch][n] (any shape of that size), weight_batch = batch or 1, NTT form under the active primes in their order; None is w = 1.
"Any words" are reduced below q before they are used."""
import numpy as np

from gpu_util import ntt_pi
from rns_ref import active_of, digits_of, mod_down_ntt, oracle_forward_set, oracle_inverse_set, product, ternary


def _weight(weight, A, batch, n):
    """[A][batch or 1][n] uint64, or None"""
    if weight is None:
        return None
    weight = np.asarray(weight, dtype=np.uint64)
    assert weight.size in (A * n, A * batch * n), weight.shape
    return weight.reshape(A, -1, n)


def accumulate_ref(n, moduli, shape, ext, key, weight, acc_old, batch, g):
    """ext [digits][A][batch n], key [digits][2][A][n], weight (above), acc_old [2][A][batch n] or None (accumulate = 0), any words -> acc [2][A][batch n]
    uint64, by the per-word definition: acc_o = (acc_old_o + w (sum_d ext_d[pi_g] key_{d,o} mod q)) mod q"""
    active = active_of(moduli, shape)
    A, D = len(active), len(digits_of(shape))
    key = np.asarray(key, dtype=np.uint64).reshape(D, 2, A, 1, n)
    gathered = np.asarray(ext, dtype=np.uint64).reshape(D, A, batch, n)[..., ntt_pi(n, g)]
    w = _weight(weight, A, batch, n)
    old = None if acc_old is None else np.asarray(acc_old, dtype=np.uint64).reshape(2, A, batch, n)
    out = np.empty((2, A, batch, n), dtype=np.uint64)
    for o in range(2):
        for j, q in enumerate(active):
            qq = np.uint64(q)
            t = np.zeros((batch, n), dtype=object)
            for d in range(D):
                t = t + (gathered[d, j] % qq).astype(object) * (key[d, o, j] % qq).astype(object)
            t = t % int(q)
            if w is not None:
                t = t * (w[j] % qq).astype(object)      # [batch or 1][n] broadcasts over the frames
            if old is not None:
                t = t + (old[o, j] % qq).astype(object)
            out[o, j] = (t % int(q)).astype(np.uint64)
    return out.reshape(2, A, batch * n)


def mul_add_ref(n, moduli, w, b, c_old, batch, g):
    """agx_ntt_mul_add_galois over `moduli` (the primes of the call's range): w [P][batch or 1][n], b [P][batch][n], c_old [P][batch][n] or None, any words
    -> c [P][batch][n] uint64: c = (c_old + w o b[pi_g]) mod q"""
    P = len(moduli)
    w = np.asarray(w, dtype=np.uint64).reshape(P, -1, n)
    b = np.asarray(b, dtype=np.uint64).reshape(P, batch, n)[..., ntt_pi(n, g)]
    old = None if c_old is None else np.asarray(c_old, dtype=np.uint64).reshape(P, batch, n)
    out = np.empty((P, batch, n), dtype=np.uint64)
    for p, q in enumerate(moduli):
        qq = np.uint64(q)
        t = (w[p] % qq).astype(object) * (b[p] % qq).astype(object)
        if old is not None:
            t = t + (old[p] % qq).astype(object)
        out[p] = (t % int(q)).astype(np.uint64)
    return out


def mod_down_pair_ref(orc, n, moduli, shape, acc):
    """agx_ntt_keyswitch_mod_down: acc [2][A][batch n] (any words) -> out [2][q_count][batch n]"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q, special = active[:q_count], active[q_count:]
    acc = np.asarray(acc, dtype=np.uint64).reshape(2, len(active), -1)
    return np.stack([mod_down_ntt(orc, n, acc[o, :q_count], acc[o, q_count:], special, Q) for o in range(2)])


def rotation_keys(orc, n, moduli, shape, elements, seed):
    """(s, shat [A][n], {g: key [digits][2][A][n]}): ONE ternary s of Hamming weight 8 and, for every Galois element, the noise-free key of
    rns_ref.rotation_key_case for sigma_g(s) -> s with random a_d of its own: key_{d,1} = a_d, key_{d,0} = -a_d s + D_P G_d sigma_g(s)"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q, A, digs = active[:q_count], len(active), digits_of(shape)
    Qp, DP = product(Q), product(active[q_count:])
    rng = np.random.default_rng(seed)
    s = ternary(rng, n, 8)
    shat = oracle_forward_set(orc, n, active, np.stack([(s % int(q)).astype(np.uint64) for q in active]))
    keys = {}
    for g in elements:
        rotated = shat[:, ntt_pi(n, g)]      # the NTT form of sigma_g(s)
        key = np.empty((len(digs), 2, A, n), dtype=np.uint64)
        for d, (first, count) in enumerate(digs):
            Dd = product(Q[first:first + count])
            G = (Qp // Dd) * pow(Qp // Dd, -1, Dd)
            for j, q in enumerate(active):
                ahat = rng.integers(0, int(q), size=n, dtype=np.uint64)
                key[d, 1, j] = ahat
                key[d, 0, j] = ((DP * G % int(q)) * rotated[j].astype(object) - ahat.astype(object) * shat[j].astype(object)) % int(q)
        keys[g] = key
    return s, shat, keys


def transform_deviation(orc, n, moduli, shape, batch, chat, shat, out, rotations, c0hat=None, diagonal=None):
    """the largest |coefficient| of out_0 + out_1 s - sum_r w_r sigma_{g_r}(c) sigma_{g_r}(s), CRT-centred modulo Q, as rns_ref.rotation_deviation centres;
    out [2][q_count][batch][n], chat [q_count][batch][n], rotations [(g, key, weight [A][1 or batch][n])]: the weight's first q_count slabs are W_r mod Q.
    With c0hat the message also holds sum_r w_r sigma_{g_r}(c0), and with `diagonal` the unrotated term diagonal (c0 + c s)"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q = active[:q_count]
    Qp = product(Q)
    out = np.asarray(out, dtype=np.uint64).reshape(2, q_count, batch, n)
    chat = np.asarray(chat, dtype=np.uint64).reshape(q_count, batch, n)
    c0 = None if c0hat is None else np.asarray(c0hat, dtype=np.uint64).reshape(q_count, batch, n)
    dhat = []
    for j, q in enumerate(Q):
        d = out[0, j].astype(object) + out[1, j].astype(object) * shat[j].astype(object)
        for g, _, weight in rotations:
            pi = ntt_pi(n, g)
            w = _weight(weight, len(active), batch, n)[j]
            d = d - (w % np.uint64(q)).astype(object) * chat[j][:, pi].astype(object) * shat[j][pi].astype(object)
            if c0hat is not None:
                d = d - (w % np.uint64(q)).astype(object) * c0[j][:, pi].astype(object)
        if diagonal is not None:
            w0 = _weight(diagonal, len(active), batch, n)[j]
            d = d - (w0 % np.uint64(q)).astype(object) * (c0[j].astype(object) + chat[j].astype(object) * shat[j].astype(object))
        dhat.append((d % int(q)).astype(np.uint64))
    res = oracle_inverse_set(orc, n, Q, np.stack(dhat))
    X = np.zeros(batch * n, dtype=object)
    for j, q in enumerate(Q):
        X = X + res[j].astype(object) * ((Qp // int(q)) * pow(Qp // int(q), -1, int(q)))
    X = X % Qp
    return max(abs(int(x) - Qp if int(x) > Qp // 2 else int(x)) for x in X)


def linear_transform_ref(orc, n, moduli, shape, ext, rotations, batch, c0hat=None, c1hat=None, diagonal=None):
    """out [2][q_count][batch][n] of the double-hoisted transform: ModDown ONCE of acc = sum_r w_r o sum_d pi_{g_r}(ext_d) o key_r, accumulated rotation by
    rotation; then, with c0hat [q_count][batch][n], out_0 += w_r[:q_count] o pi_{g_r}(c0hat) for every rotation; then, with `diagonal` (a weight) and
    c1hat, the unrotated term out_0 += diagonal o c0hat, out_1 += diagonal o c1hat.  rotations: [(g, key, weight)], weight not None when c0hat is given"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    A, Q = len(active), active[:q_count]
    acc = None
    for g, key, weight in rotations:
        acc = accumulate_ref(n, moduli, shape, ext, key, weight, acc, batch, g)
    out = mod_down_pair_ref(orc, n, moduli, shape, acc).reshape(2, q_count, batch, n)
    if c0hat is not None:
        for g, _, weight in rotations:
            out[0] = mul_add_ref(n, Q, _weight(weight, A, batch, n)[:q_count], c0hat, out[0], batch, g)
    if diagonal is not None:
        w0 = _weight(diagonal, A, batch, n)[:q_count]
        out[0] = mul_add_ref(n, Q, w0, c0hat, out[0], batch, 1)
        out[1] = mul_add_ref(n, Q, w0, c1hat, out[1], batch, 1)
    return out
