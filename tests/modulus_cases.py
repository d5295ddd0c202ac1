"""Moduli away from the top of their arithmetic class, computed from the CPU oracle at test time: the primes next to every bound a class predicate of
the library compares against (2^30, 2^31, 2^32, 2^58, 2^60, 2^61, 2^60 - 2^28), the widths parameter sets of the libraries in use sit at (36, 40, 43,
44, 50, 54 bits), the smallest admitted primes, and plans of six that mix them in the order of the key-switch shapes of rns_cases.py (Q first, special
primes last).  test_modulus_cases.py judges this module on the CPU; test_gpu_modulus_classes.py feeds the device with it.  Results are computed once
and read-only; nothing here skips: what cannot be formed raises.  It imports from gpu_util only."""
import functools

from gpu_util import PRODUCT_IDS, REGISTRY

LIMIT = 1 << 62      # check_modulus admits odd q < 2^62 with 2n | q - 1
C_BOUND = (1 << 60) - (1 << 28)      # 2^60 - c with 0 < c < 2^28 lies strictly above it
CLASS_BOUNDS = (30, 31, 32, 58, 60, 61)      # log2 of the bounds that have a prime on either side in edge_moduli
WIDTHS = (36, 40, 43, 50, 54)      # mid-width primes, the largest below 2^bits each


@functools.lru_cache(maxsize=None)
def prime_above(orc, bound, n, k=0):
    """the k-th prime = 1 (mod 2n) strictly above `bound`, stepping by 2n; raises past the admitted range"""
    step = 2 * n
    c = bound // step * step + 1
    if c <= bound:
        c += step
    while True:
        if c >= LIMIT:
            raise ValueError(f"no admitted prime number {k} above {bound} at n = {n}")
        if orc.is_prime(c):
            if k == 0:
                return c
            k -= 1
        c += step


@functools.lru_cache(maxsize=None)
def prime_below(orc, bound, n, k=0):
    """the k-th prime = 1 (mod 2n) strictly below `bound`, stepping by 2n; raises when there is none"""
    step = 2 * n
    c = (bound - 1) // step * step + 1
    if c >= bound:
        c -= step
    while True:
        if c < 3:
            raise ValueError(f"no admitted prime number {k} below {bound} at n = {n}")
        if c < LIMIT and orc.is_prime(c):
            if k == 0:
                return c
            k -= 1
        c -= step


@functools.lru_cache(maxsize=None)
def _edges(orc, n):
    e = {"min": prime_above(orc, 1, n)}
    for b in CLASS_BOUNDS:
        e[f"below{b}"] = prime_below(orc, 1 << b, n)
        e[f"above{b}"] = prime_above(orc, 1 << b, n)
    e["below62"] = prime_below(orc, 1 << 62, n)
    e["c_max"] = prime_above(orc, C_BOUND, n)
    e["c_out"] = prime_below(orc, C_BOUND, n)
    for b in WIDTHS:
        e[f"below{b}"] = prime_below(orc, 1 << b, n)
    return e


def edge_moduli(orc, n):
    """{name: modulus}: `min` the smallest admitted prime; below<b> / above<b> the primes next to 2^b for b = 30, 31, 32, 58, 60, 61 and below62;
    c_max / c_out the primes next to 2^60 - 2^28 on the side of the class q = 2^60 - c and outside it; below36 .. below54 the mid widths"""
    return dict(_edges(orc, n))


def edge_bounds():
    """{name: (side, bound)} of every entry of edge_moduli: the prime lies strictly on `side` (+1 above, -1 below) of `bound`, nearest to it"""
    out = {"min": (1, 1), "below62": (-1, 1 << 62), "c_max": (1, C_BOUND), "c_out": (-1, C_BOUND)}
    for b in CLASS_BOUNDS:
        out[f"below{b}"], out[f"above{b}"] = (-1, 1 << b), (1, 1 << b)
    for b in WIDTHS:
        out[f"below{b}"] = (-1, 1 << b)
    return out


@functools.lru_cache(maxsize=None)
def _mixes(orc, n):
    e = _edges(orc, n)
    below = lambda bits, k=0: prime_below(orc, 1 << bits, n, k)      # noqa: E731
    above = lambda bits, k=0: prime_above(orc, 1 << bits, n, k)      # noqa: E731
    smallest = [prime_above(orc, 1, n, k) for k in range(6)]
    # the largest prime below 2^17 is `min` itself at n = 16384 and 32768 (65537): the smallest admitted prime that tier2 does not hold yet stands in
    # there (the second smallest at n = 16384; at n = 32768 that one, 786433, is the largest below 2^20, so the third)
    tier2_rest = (e["min"], e["below30"], above(29), below(20), below(25))
    narrow17 = below(17) if below(17) not in tier2_rest else next(q for q in smallest if q not in tier2_rest)
    mixes = {
        "ckks40": (below(60), below(40), below(40, 1), below(40, 2), below(60, 1), below(60, 2)),
        "seal": (below(43), below(43, 1), below(44), below(44, 1), below(50), below(54)),
        "edge60": (e["above58"], e["below58"], e["below60"], e["c_max"], e["c_out"], above(59)),
        "edge61": (e["above60"], e["below61"], e["below40"], e["min"], e["above32"], e["below60"]),
        "edge62": (e["above61"], e["below62"], e["min"], e["below40"], e["below60"], e["below61"]),
        "tiny": tuple(smallest),
        "tier2": (e["min"], e["below30"], above(29), narrow17, below(20), below(25)),
        "tier1": (e["above30"], e["below31"], e["min"], e["below30"], below(20), below(25)),
        "over31": (e["above31"], e["below32"], e["min"], e["below30"], e["below31"], e["above32"]),
    }
    for name, m in mixes.items():
        if len(set(m)) != 6:
            raise ValueError(f"mix {name} has no six distinct moduli at n = {n}: {m}")
    return mixes


def MIXES(orc, n):
    """{name: six distinct moduli}, Q first and the special primes last (rns_cases.TOP / LOWER): ckks40 (16q-lazy class, estimate and four-step primes
    in one plan), seal (16q-lazy, four-step only), edge60 (both sides of 2^58 and of 2^60 - 2^28), edge61 (fast class, the smallest prime next to
    61-bit ones), edge62 (exact class), tiny (the six smallest admitted primes), tier2 / tier1 (the 32-bit tiers from their lower edges up) and over31
    (narrow-looking moduli that the 64-bit kernels must serve)"""
    return dict(_mixes(orc, n))


MIX_NAMES = ("ckks40", "seal", "edge60", "edge61", "edge62", "tiny", "tier2", "tier1", "over31")


def admits(max_bits, moduli):
    """whether a registry entry of `max_bits` admits every modulus: the 32-bit tiers need all q < 2^30 / 2^31, the 64-bit classes all q <= 2^60 /
    2^61 / any admitted q"""
    if max_bits in (30, 31):
        return all(q < 1 << max_bits for q in moduli)
    if max_bits in (60, 61):
        return all(q <= 1 << max_bits for q in moduli)
    if max_bits == 62:
        return all(q < LIMIT for q in moduli)
    raise ValueError(f"unknown class {max_bits}")


def expected_class(n, moduli):
    """the max_bits of the entry a default plan must choose: the smallest among the product library's registry entries of size n that admit every modulus"""
    classes = sorted({bits for config, size, bits in REGISTRY if size == n and config in PRODUCT_IDS})
    for bits in classes:
        if admits(bits, moduli):
            return bits
    raise ValueError(f"no registry entry of size {n} admits {moduli}")
