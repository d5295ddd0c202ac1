"""What the tests of the ring calls (agx_ntt_add, _sub, _negate, _add_galois, _tensor) share: their Python-integer reference model over dense frame
sets, operands drawn once per shape, and the two compositions they complete -- a homomorphic multiplication (tensor, key switch of c_2 with a key for
s^2 -> s, two adds) and a hoisted rotation (decompose, apply_decomposed, add_galois) -- with their noise conditions.  test_ring_reference.py judges this
module on the CPU; test_gpu_ring_ops.py judges the device against it.  It imports from gpu_util and rns_ref only."""
import functools

import numpy as np

from gpu_util import ntt_pi
from rns_ref import (active_of, digits_of, hoisted_ref, keyswitch_ref, oracle_forward_set, oracle_inverse_set, product, rotation_key_case, spread,
                     ternary)


# ---- the reference model: frame sets [P][B][n] (any 64-bit words: reduced first), slab p under moduli[p]; Python integers throughout -------------
def _residues(x, p, q):
    return (np.asarray(x[p], dtype=np.uint64) % np.uint64(q)).astype(object)


def _words(slabs, q):
    return (slabs % int(q)).astype(np.uint64)


def add_ref(a, b, moduli):
    return np.stack([_words(_residues(a, p, q) + _residues(b, p, q), q) for p, q in enumerate(moduli)])


def sub_ref(a, b, moduli):
    return np.stack([_words(_residues(a, p, q) - _residues(b, p, q), q) for p, q in enumerate(moduli)])


def neg_ref(a, moduli):
    return np.stack([_words(-_residues(a, p, q), q) for p, q in enumerate(moduli)])


def add_galois_ref(a, b, moduli, g):
    """c[p][f][i] = a[p][f][i] + b[p][f][pi_g(i)], pi_g = gpu_util.ntt_pi: the permutation of agx_ntt_automorphism(AGX_FORM_NTT)"""
    n = np.asarray(b).shape[-1]
    return add_ref(a, np.asarray(b)[..., ntt_pi(n, g)], moduli)


def tensor_ref(a, b, moduli):
    """a, b [2][P][B][n] -> [3][P][B][n]: (a_0 b_0, a_0 b_1 + a_1 b_0, a_1 b_1) mod q"""
    out = []
    for p, q in enumerate(moduli):
        a0, a1, b0, b1 = _residues(a[0], p, q), _residues(a[1], p, q), _residues(b[0], p, q), _residues(b[1], p, q)
        out.append(np.stack([_words(a0 * b0, q), _words(a0 * b1 + a1 * b0, q), _words(a1 * b1, q)]))
    return np.stack(out, axis=1)


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ring_operands(n, moduli, batch, seed):
    """(a, b) [2][P][batch][n] reduced and the same spread over [0, 4q), drawn once per shape (read-only): the linear calls take component 0 of each.
    Every prime's first frame opens with 0, q - 1, q - 1, 1 in a and q - 1, q - 1, 0, q - 1 in b: -0, (q - 1) + (q - 1), 0 - (q - 1), (q - 1)^2"""
    rng = np.random.default_rng(seed)
    a = np.stack([rng.integers(0, q, size=(2, batch, n), dtype=np.uint64) for q in moduli], axis=1)
    b = np.stack([rng.integers(0, q, size=(2, batch, n), dtype=np.uint64) for q in moduli], axis=1)
    top = np.array(moduli, dtype=np.uint64) - np.uint64(1)
    k = min(n, 4)
    a[:, :, 0, :k] = np.stack([np.zeros_like(top), top, top, np.ones_like(top)], axis=1)[None, :, :k]
    b[:, :, 0, :k] = np.stack([top, top, np.zeros_like(top), top], axis=1)[None, :, :k]
    out = (a, b, spread(rng, a, moduli, 1), spread(rng, b, moduli, 1))
    for w in out:
        w.setflags(write=False)
    return out


# ---- noise: the CRT-centred size of an NTT-form frame set ---------------------------------------------------------------------------------------
def centred_deviation(orc, n, Q, dhat):
    """the largest |coefficient| of the polynomials with NTT form dhat [len(Q)][count] under Q, CRT-centred modulo prod Q"""
    res = oracle_inverse_set(orc, n, Q, dhat)
    Qp = product(Q)
    X = np.zeros(res.shape[1], dtype=object)
    for j, q in enumerate(Q):
        X = X + res[j].astype(object) * ((Qp // int(q)) * pow(Qp // int(q), -1, int(q)))
    X = X % Qp
    return max(abs(int(x) - Qp if int(x) > Qp // 2 else int(x)) for x in X)


def _encrypt(rng, Q, mhat, shat, batch, n):
    """(c_0, c_1) [2][len(Q)][batch][n] with c_1 random and c_0 = mhat - c_1 shat: a noise-free ciphertext of m under s, in NTT form"""
    c1 = np.stack([rng.integers(0, int(q), size=(batch, n), dtype=np.uint64) for q in Q])
    c0 = np.stack([_words(mhat[j].astype(object) - c1[j].astype(object) * shat[j].astype(object), q) for j, q in enumerate(Q)])
    return np.stack([c0, c1])


# ---- homomorphic multiplication -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hmult_case(orc, n, moduli, shape, batch, seed):
    """(a, b [2][q_count][batch][n], key [digits][2][A][n], s, shat [A][n], mhat, mhat' [q_count][batch][n]): two noise-free ciphertexts of random m, m'
    under a ternary s of weight 8, and the noise-free key for s^2 -> s: key_{d,1} = a_d random, key_{d,0} = -a_d s + D_P G_d s^2 with G_d = (Q / D_d)
    [(Q / D_d)^-1 mod D_d] -- rns_ref.rotation_key_case with shat o shat in the place of the rotated shat.  Everything in NTT form, read-only"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q, A, digs = active[:q_count], len(active), digits_of(shape)
    Qp, DP = product(Q), product(active[q_count:])
    rng = np.random.default_rng(seed)
    s = ternary(rng, n, 8)
    shat = oracle_forward_set(orc, n, active, np.stack([(s % int(q)).astype(np.uint64) for q in active]))
    squared = np.stack([_words(shat[j].astype(object) * shat[j].astype(object), q) for j, q in enumerate(active)])      # the NTT form of s^2
    key = np.empty((len(digs), 2, A, n), dtype=np.uint64)
    for d, (first, count) in enumerate(digs):
        Dd = product(Q[first:first + count])
        G = (Qp // Dd) * pow(Qp // Dd, -1, Dd)
        for j, q in enumerate(active):
            ahat = rng.integers(0, int(q), size=n, dtype=np.uint64)
            key[d, 1, j] = ahat
            key[d, 0, j] = ((DP * G % int(q)) * squared[j].astype(object) - ahat.astype(object) * shat[j].astype(object)) % int(q)
    mhat = [np.stack([rng.integers(0, int(q), size=(batch, n), dtype=np.uint64) for q in Q]) for _ in range(2)]
    shat_frames = shat[:q_count, None, :]
    out = (_encrypt(rng, Q, mhat[0], shat_frames, batch, n), _encrypt(rng, Q, mhat[1], shat_frames, batch, n), key, s, shat, mhat[0], mhat[1])
    for w in out:
        w.setflags(write=False)
    return out


def hmult_ref(orc, n, moduli, shape, a, b, key, batch):
    """the composition on the reference alone: d = tensor_ref(a, b); out = keyswitch_ref(d_2); (out_0 + d_0, out_1 + d_1), [2][q_count][batch][n]"""
    q_count = shape[0]
    Q = active_of(moduli, shape)[:q_count]
    d = tensor_ref(np.asarray(a).reshape(2, q_count, batch, n), np.asarray(b).reshape(2, q_count, batch, n), Q)
    out = keyswitch_ref(orc, n, moduli, shape, d[2], key, batch)
    return np.stack([add_ref(out[0], d[0], Q), add_ref(out[1], d[1], Q)])


def hmult_deviation(orc, n, moduli, shape, batch, r, shat, mhat, mhat2):
    """the largest |coefficient| of r_0 + r_1 s - m m', CRT-centred modulo Q; r [2][q_count][batch][n]"""
    q_count = shape[0]
    Q = active_of(moduli, shape)[:q_count]
    r = np.asarray(r, dtype=np.uint64).reshape(2, q_count, batch, n)
    dhat = np.stack([_words(r[0, j].astype(object) + r[1, j].astype(object) * shat[j].astype(object) - mhat[j].astype(object) * mhat2[j].astype(object), q)
                     for j, q in enumerate(Q)])
    return centred_deviation(orc, n, Q, dhat)


# ---- hoisted rotation ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hrotate_case(orc, n, moduli, shape, g, batch, seed):
    """(c [2][q_count][batch][n], key, s, shat, mhat): rns_ref.rotation_key_case's c_1, key and s, and c_0 = mhat - c_1 shat for a random m (read-only)"""
    q_count = shape[0]
    Q = active_of(moduli, shape)[:q_count]
    c1, key, s, shat = rotation_key_case(orc, n, moduli, shape, g, batch, seed)
    rng = np.random.default_rng(seed + 1)
    mhat = np.stack([rng.integers(0, int(q), size=(batch, n), dtype=np.uint64) for q in Q])
    c0 = np.stack([_words(mhat[j].astype(object) - c1[j].astype(object) * shat[j].astype(object), q) for j, q in enumerate(Q)])
    out = (np.stack([c0, c1]), key, s, shat, mhat)
    for w in out:
        w.setflags(write=False)
    return out


def hrotate_ref(orc, n, moduli, shape, c, key, batch, g):
    """hoisted_ref on c_1, then out_0 += pi_g(c_0): [2][q_count][batch][n]"""
    q_count = shape[0]
    Q = active_of(moduli, shape)[:q_count]
    c = np.asarray(c).reshape(2, q_count, batch, n)
    out = hoisted_ref(orc, n, moduli, shape, c[1], key, batch, g)
    return np.stack([add_galois_ref(out[0], c[0], Q, g), out[1]])


def hrotate_deviation(orc, n, moduli, shape, g, batch, r, shat, mhat):
    """the largest |coefficient| of r_0 + r_1 s - sigma_g(m), CRT-centred modulo Q"""
    q_count = shape[0]
    Q = active_of(moduli, shape)[:q_count]
    r = np.asarray(r, dtype=np.uint64).reshape(2, q_count, batch, n)
    pi = ntt_pi(n, g)
    dhat = np.stack([_words(r[0, j].astype(object) + r[1, j].astype(object) * shat[j].astype(object) - mhat[j][:, pi].astype(object), q) for j, q in enumerate(Q)])
    return centred_deviation(orc, n, Q, dhat)
