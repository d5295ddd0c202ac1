"""CPU tests of the case helpers of gpu_util.py that the GPU tests share: moduli by width and rank, the cached oracle tables, the registry
tables, status_of.  n = 64 throughout; no device is needed."""
import numpy as np

from gpu_util import (PRODUCT_IDS, REGISTRY, RESCALE_IDS, library_find_prime, moduli_for, oracle_forward_rns, oracle_tables, registry_entries,
                      status_of, tables_for)

N = 64


def test_moduli_by_width_and_rank_are_the_primes_of_tables_for(orc):
    """[60, 30, 60]: the largest 60-bit prime, the largest 30-bit prime, the second largest 60-bit prime"""
    moduli = moduli_for(orc.find_prime, N, [60, 30, 60])
    t60, t30 = tables_for(orc, N, 60, 2), tables_for(orc, N, 30, 1)
    assert moduli == (t60[0][0], t30[0][0], t60[1][0])
    assert moduli[0] > moduli[2] > 1 << 59 and moduli[1] < 1 << 30


def test_the_librarys_finder_gives_the_same_moduli(agx, orc):
    assert moduli_for(library_find_prime(agx), N, [60, 30, 60]) == moduli_for(orc.find_prime, N, [60, 30, 60])


def test_oracle_tables_are_cached_and_read_only(orc):
    q = orc.find_prime(60, N)
    t = oracle_tables(orc, N, q)
    assert oracle_tables(orc, N, q) is t and tables_for(orc, N, 60)[0] is t
    assert t[:2] == (q, orc.min_root(q, N))
    tw, pre = orc.make_tables(q, t[1], N)
    assert np.array_equal(t[2], tw) and np.array_equal(t[3], pre)
    assert not t[2].flags.writeable and not t[3].flags.writeable


def test_oracle_forward_rns_is_the_oracles_forward_per_prime(orc):
    tabs = [oracle_tables(orc, N, q) for q in moduli_for(orc.find_prime, N, [60, 30])]
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.integers(0, t[0], size=3 * N, dtype=np.uint64) for t in tabs])
    want = np.concatenate([orc.forward(x[p * 3 * N:(p + 1) * 3 * N], t[0], t[2], t[3], N) for p, t in enumerate(tabs)])
    assert np.array_equal(oracle_forward_rns(orc, x, tabs, N), want)
    assert np.array_equal(oracle_forward_rns(orc, x.reshape(2, 3, N), tabs, N), want)


def test_registry_ids_are_unique():
    ids = [e[0] for e in REGISTRY]
    assert len(ids) == len(set(ids)) == 86


def test_rescale_ids_are_registry_entries():
    ids = {e[0] for e in REGISTRY}
    assert set(RESCALE_IDS) <= ids and set(RESCALE_IDS) <= PRODUCT_IDS and len(set(RESCALE_IDS)) == len(RESCALE_IDS) == 18
    assert [e[0] for e in registry_entries(RESCALE_IDS)] == RESCALE_IDS
    assert [e[1:] for e in registry_entries([117, 91])] == [(16384, 60), (4096, 62)]      # in the order asked for, (n, max_bits) from REGISTRY


def test_product_ids_and_the_registry_differ_by_the_ab_entries_alone():
    ids = {e[0] for e in REGISTRY}
    assert PRODUCT_IDS - ids == set()
    assert ids - PRODUCT_IDS == {70, 114, 115, 147, 160, 161, 215, 220, 221, 222, 224, 235, 236}      # lib/libagxntt_diag.so only


def test_status_of(agx):
    assert status_of(agx, lambda *a: None, 1, 2) == 0
    assert status_of(agx, agx.find_primes, 63, N) == 5      # q must stay below 2^62
    assert status_of(agx, agx.min_root, 97, N) == 3         # 96 is not divisible by 128
