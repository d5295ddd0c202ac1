"""The Python reference of the hoisted key switch (agx_ntt_keyswitch_decompose + agx_ntt_keyswitch_apply_decomposed), shared by the CPU test of the
reference alone and the device tests.  It is tests/test_gpu_keyswitch.py's four-step reference cut in two, with every NTT-form digit read through
pi_g = gpu_util.ntt_pi(n, g) per frame in step 3; and the noise-free rotation key with which the call must switch sigma_g(c) from sigma_g(s) to s."""
import numpy as np

from gpu_util import ntt_pi
from test_gpu_keyswitch import _fwd, _inv, _product, _residues, _ternary, active_of, digits_of, lift


def decompose_ref(orc, n, moduli, shape, chat):
    """steps 1 and 2: chat [q_count][batch][n] (any words below 4q) -> ext [digits][A][batch n] uint64, fully reduced"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q = active[:q_count]
    c = _inv(orc, n, Q, chat)
    return np.stack([_fwd(orc, n, active, _residues(lift(c[first:first + count], Q[first:first + count]), active)) for first, count in digits_of(shape)])


def apply_decomposed_ref(orc, n, moduli, shape, ext, key, batch, g):
    """steps 3 and 4 with ext read through pi_g: ext [digits][A][batch n], key [digits][2][A][n] (any words below 4q) -> out [2][q_count][batch][n]"""
    q_count = shape[0]
    active = active_of(moduli, shape)
    Q, special = active[:q_count], active[q_count:]
    A, D = len(active), len(digits_of(shape))
    key = np.asarray(key, dtype=np.uint64).reshape(D, 2, A, 1, n)
    gathered = np.asarray(ext, dtype=np.uint64).reshape(D, A, batch, n)[..., ntt_pi(n, g)]
    out = []
    DP = _product(special)
    for o in range(2):
        acchat = []
        for j, q in enumerate(active):
            s = np.zeros((batch, n), dtype=object)
            for d in range(D):
                s = s + gathered[d, j].astype(object) * (key[d, o, j] % np.uint64(q)).astype(object)
            acchat.append((s % int(q)).astype(np.uint64).reshape(-1))
        acchat = np.stack(acchat)
        a, V = _inv(orc, n, Q, acchat[:q_count]), lift(_inv(orc, n, special, acchat[q_count:]), special)
        coeff = np.stack([((a[j].astype(object) - V) * pow(DP, -1, int(q)) % int(q)).astype(np.uint64) for j, q in enumerate(Q)])
        out.append(_fwd(orc, n, Q, coeff))
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
    Qp, DP = _product(Q), _product(active[q_count:])
    rng = np.random.default_rng(seed)
    s = _ternary(rng, n, 8)
    shat = _fwd(orc, n, active, np.stack([(s % int(q)).astype(np.uint64) for q in active]))
    rotated = shat[:, ntt_pi(n, g)]      # the NTT form of sigma_g(s)
    key = np.empty((len(digs), 2, A, n), dtype=np.uint64)
    for d, (first, count) in enumerate(digs):
        Dd = _product(Q[first:first + count])
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
    Qp = _product(Q)
    pi = ntt_pi(n, g)
    out = np.asarray(out, dtype=np.uint64).reshape(2, q_count, batch, n)
    dhat = np.stack([((out[0, j].astype(object) + out[1, j].astype(object) * shat[j].astype(object)
                       - chat[j][:, pi].astype(object) * shat[j][pi].astype(object)) % int(q)).astype(np.uint64) for j, q in enumerate(Q)])
    res = _inv(orc, n, Q, dhat)
    X = np.zeros(batch * n, dtype=object)
    for j, q in enumerate(Q):
        X = X + res[j].astype(object) * ((Qp // int(q)) * pow(Qp // int(q), -1, int(q)))
    X = X % Qp
    return max(abs(int(x) - Qp if int(x) > Qp // 2 else int(x)) for x in X)


def rotation_bound(shape, s):
    """p_count (1 + ||s||_1): what the two approximate conversions leave, a condition and not a measurement (test_it_switches_keys)"""
    return shape[2] * (1 + int(np.abs(s).sum()))
