"""Regenerates tests/golden/q60c_boundary.json: the 60-bit NTT primes q = 2^60 - c = 1 (mod 8192) with the smallest and the largest
c below 2^28 (the class of moduli of the forward kernel registry id 165), their smallest primitive 8192nd roots, and the oracle's forward
transform of one frame each (inputs: oracle.fill_splitmix(n, seed, q)).  Run from the repository root: python tests/golden/make_q60c_boundary.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as orc  # noqa: E402

N, SEED = 4096, 60


def boundary_primes(n=N):
    """(smallest c, largest c): search down from 2^60 and up from 2^60 - 2^28 over q = 1 (mod 2n)"""
    top, step = 1 << 60, 2 * n
    q = top - step + 1
    while not orc.is_prime(q):
        q -= step
    lo = q
    q = top - (1 << 28)
    q += (1 - q) % step
    while top - q >= (1 << 28) or not orc.is_prime(q):
        q += step
    return lo, q


if __name__ == "__main__":
    cases = []
    for q in boundary_primes():
        psi = orc.min_root(q, N)
        tw, pre = orc.make_tables(q, psi, N)
        y = orc.forward(orc.fill_splitmix(N, SEED, q), q, tw, pre, N)
        cases.append({"q": q, "c": (1 << 60) - q, "psi": psi, "seed": SEED, "forward_hex": [format(int(v), "x") for v in y]})
    with open(os.path.join(ROOT, "tests", "golden", "q60c_boundary.json"), "w") as f:
        json.dump({"n": N, "cases": cases}, f, separators=(",", ":"))
    print([(c["q"], c["c"]) for c in cases])
