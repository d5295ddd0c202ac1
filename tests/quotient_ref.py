"""The Python-integer model of agx_ntt_basis_quotient, stated on tests/bfv_conv_ref.py as it stands, and the cases the tests of that call share.  The model
is steps 4 to 7 of the INTEGRATION.md listing in coefficient form: times t, ModDown with sources Q and targets Bsk (the fast floor), extend_exact from B to Q
through m.  A frame set is what bfv_conv_ref takes: [len(moduli)][count] integers, any words."""
import bfv_conv_ref as ref


def floor_on_bsk(x, Q, B, m, t):
    """x [L + K + 1][count], rows under Q, then B, then m -> f [K + 1][count] under B, then m: ((t x_j') - V) D^-1 mod b_j with V the lift of the Q rows"""
    L, every = len(Q), tuple(Q) + tuple(B) + (m,)
    tx = [[t * (v % q) for v in row] for row, q in zip(x, every)]
    return ref.mod_down(tx[L:], tx[:L], tuple(Q), tuple(B) + (m,))


def quotient(x, Q, B, m, t):
    """the contract's words in coefficient form: x [L + K + 1][count] -> [L][count]"""
    K = len(B)
    f = floor_on_bsk(x, Q, B, m, t)
    return ref.extend_exact(f[:K], f[K], tuple(B), tuple(Q), m)


def alphas(x, Q, B, m, t):
    """the alpha of every coefficient, in [-(m - 1) / 2, (m - 1) / 2]"""
    K = len(B)
    f = floor_on_bsk(x, Q, B, m, t)
    return ref.alpha_exact(f[:K], f[K], tuple(B), m)[1]


def rows_with_alphas(rng, Q, B, m, t, count, wanted):
    """Reduced coefficient-form rows [L + K + 1][count]: the Q and B rows random with the ends of the residue range in front, the m row CONSTRUCTED so that
    coefficient e has alpha = wanted[e % len(wanted)] (None: a random word).  f_m -> a_m is a bijection modulo m when t is invertible there:
    t a_m = f_m D + V and f_m = W - alpha B (mod m).  rng: numpy's Generator."""
    assert t % m
    Q, B = tuple(Q), tuple(B)
    L, K = len(Q), len(B)
    rows = [[int(v) for v in rng.integers(0, q, size=count, dtype="uint64")] for q in Q + B]
    for row, q in zip(rows, Q + B):
        row[0], row[1 % count] = 0, q - 1
    D, Bp = ref.product(Q), ref.product(B)
    tq = [[t * v for v in row] for row in rows[:L]]
    V = ref.lift(tq, Q)
    f = ref.mod_down([[t * v for v in row] for row in rows[L:]], tq, Q, B)
    W = ref.lift(f, B)
    am = []
    for e in range(count):
        alpha = wanted[e % len(wanted)]
        if alpha is None:
            am.append(int(rng.integers(0, m, dtype="uint64")))
        else:
            assert 2 * abs(alpha) <= m - 1
            am.append(((W[e] - alpha * Bp) * D + V[e]) * pow(t, -1, m) % m)
    return rows + [am]
