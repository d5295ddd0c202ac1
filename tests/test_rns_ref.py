"""The parts of the tests' reference model (tests/rns_ref.py) against each other, no device, at n = 8 and 64: convert is residues(lift), ModDown
from one source is the rescale in floor mode, the regions of test_gpu_mod_down's inputs whose result is known in closed form hold, and lift,
oracle_inverse_set and spread give the words of each variant the GPU test files used to carry (written out here).  The key switch's references are
held against each other by tests/test_hoist_reference.py."""
import numpy as np
import pytest

from gpu_util import moduli_for, oracle_tables, rescale_reference
from rns_cases import MIXED_WIDTHS, SWEEP_PRIMES, extend_shape, mod_down_shape
from rns_ref import convert, lift, mod_down, oracle_forward_set, oracle_inverse_set, product, residues, special_values, spread

SIZES = (8, 64)
WIDE_SOURCE_COUNTS = (5, 8, 9, 15)      # inside and at the ends of the kernels' source capacities 8 and 16 (test_gpu_source_counts.py sweeps 1 ... 16)


def _bases(orc, n):
    """(source moduli, target moduli) of mixed widths: one, two and three sources, targets that contain the sources and targets apart from them"""
    m = moduli_for(orc.find_prime, n, [60, 30, 61, 30, 60, 60])
    return [(m[2:3], m), (m[1:3], m), (m[4:6], m[:4]), (m[3:6], m[:3])]


def _wide_bases(orc, n, S):
    """the bases of test_gpu_source_counts.py at S sources on 19 primes, all 60-bit and of mixed widths: [extend's (the first target is the last source),
    ModDown's (targets apart from the sources)] per plan"""
    out = []
    for widths in ([60] * SWEEP_PRIMES, MIXED_WIDTHS):
        m = moduli_for(orc.find_prime, n, widths)
        out += [(m[sf:sf + sc], m[df:df + dc]) for sf, sc, df, dc in (extend_shape(S), mod_down_shape(S))]
    return out


def _random_residues(rng, moduli, count):
    return np.stack([rng.integers(0, int(q), size=count, dtype=np.uint64) for q in moduli])


@pytest.mark.parametrize("n", SIZES)
def test_convert_is_the_residues_of_the_lift(orc, n):
    """on the special values and on random residues, reduced and spread over [0, 4q): out_j = V mod q_j with V = X + u D, 0 <= u < S; a target that is
    a source gets its residue back"""
    _check_convert(np.random.default_rng(n), n, _bases(orc, n))


@pytest.mark.parametrize("S", WIDE_SOURCE_COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_convert_is_the_residues_of_the_lift_at_wide_source_counts(orc, n, S):
    """the same properties on the sweep's bases: S = 5, 8, 9, 15 sources"""
    _check_convert(np.random.default_rng(n + S), n, _wide_bases(orc, n, S))


def _check_convert(rng, n, bases):
    for src, dst in bases:
        D, special = product(src), special_values(src)
        x = np.concatenate([residues(special, src), _random_residues(rng, src, 4 * n)], axis=1)
        V = lift(x, src)
        assert all(int(v) % D == X and int(v) // D < len(src) for v, X in zip(V[:len(special)], special))
        got = convert(x, src, dst)
        assert got.dtype == np.uint64 and got.shape == (len(dst), x.shape[1])
        assert np.array_equal(got, residues(V, dst)) and np.array_equal(got, residues([int(v) for v in V], dst))      # an object array or a list
        assert np.array_equal(got, np.array([[int(v) % int(q) for v in V] for q in dst], dtype=np.uint64))
        assert np.array_equal(convert(spread(rng, x, src), src, dst), got)
        for j, q in enumerate(dst):
            if q in src:
                assert np.array_equal(got[j], x[src.index(q)])


@pytest.mark.parametrize("n", SIZES)
def test_mod_down_from_one_source_is_the_rescale_in_floor_mode(orc, n):
    rng = np.random.default_rng(n + 1)
    for widths in ([60] * 4, [60, 30, 61, 30], [30, 60, 60]):
        moduli = moduli_for(orc.find_prime, n, widths)
        x = _random_residues(rng, moduli, 3 * n)
        x[:, :4] = np.array([[0, 1, q - 1, q // 2] for q in moduli], dtype=np.uint64)
        assert np.array_equal(mod_down(x[:-1], x[-1:], moduli[-1:], moduli[:-1]), rescale_reference(x, moduli, 0))


@pytest.mark.parametrize("n", SIZES)
def test_closed_form_regions_of_the_mod_down_inputs(orc, n):
    """X = D Y + V with V the lift of the sources gives Y mod q_j ("quotient"), and a_j = V mod q_j gives zero: the two constructions test_gpu_mod_down's
    make_inputs plants, here on random sources and on the special values"""
    _check_closed_forms(np.random.default_rng(n + 2), n, _bases(orc, n)[2:])


@pytest.mark.parametrize("S", WIDE_SOURCE_COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_closed_form_regions_of_the_mod_down_inputs_at_wide_source_counts(orc, n, S):
    """the same constructions from S = 5, 8, 9, 15 sources into three targets apart from them"""
    _check_closed_forms(np.random.default_rng(n + 2 + S), n, _wide_bases(orc, n, S)[1::2])


def _check_closed_forms(rng, n, bases):
    for src, dst in bases:
        D = product(src)
        p = np.concatenate([residues(special_values(src), src), _random_residues(rng, src, 2 * n)], axis=1)
        V = lift(p, src)
        Y = rng.integers(0, 1 << 20, size=V.size).astype(object)
        assert np.array_equal(mod_down(residues(D * Y + V, dst), p, src, dst), residues(Y, dst))
        assert not mod_down(residues(V, dst), p, src, dst).any()


@pytest.mark.parametrize("n", SIZES)
def test_the_unified_helpers_give_the_words_of_the_old_variants(orc, n):
    """on reduced inputs: lift with and without its range assertion, the inverse with and without the reduction in front, spread flattened, shape-keeping
    and along an axis"""
    rng = np.random.default_rng(n + 3)
    moduli = moduli_for(orc.find_prime, n, [60, 30, 61])
    x = _random_residues(rng, moduli, 2 * n)
    D = product(moduli)
    lift_plain = lambda p: sum(((p[i] % np.uint64(q)).astype(object) * pow(D // int(q), -1, int(q)) % int(q)) * (D // int(q))      # noqa: E731
                               for i, q in enumerate(moduli))
    assert np.array_equal(lift(x, moduli), lift_plain(x))
    inverse_of = lambda words, q: orc.inverse(np.ascontiguousarray(words), q, orc.make_inv_tables(q, oracle_tables(orc, n, q)[1], n)[0], n)      # noqa: E731
    inv_unreduced = lambda xhat: np.stack([inverse_of(xhat[i], q) for i, q in enumerate(moduli)])      # noqa: E731
    inv_reduced = lambda xhat: np.stack([inverse_of(xhat[i] % np.uint64(q), q) for i, q in enumerate(moduli)])      # noqa: E731
    got = oracle_inverse_set(orc, n, moduli, x)
    assert np.array_equal(got, inv_unreduced(x)) and np.array_equal(got, inv_reduced(x))
    assert np.array_equal(oracle_inverse_set(orc, n, moduli, spread(rng, x, moduli)), got)
    assert np.array_equal(oracle_forward_set(orc, n, moduli, got), x)
    # spread: one draw of x.shape against the per-prime sequential draws of the flattening variants, from the same generator state
    spread_flat = lambda r, w: np.stack([w[i] + np.uint64(q) * r.integers(0, 4, size=w.shape[1], dtype=np.uint64) for i, q in enumerate(moduli)])      # noqa: E731
    spread_axis = lambda r, w, axis: w + np.array(moduli, dtype=np.uint64).reshape([-1 if k == axis else 1 for k in range(w.ndim)]) * r.integers(      # noqa: E731
        0, 4, size=w.shape, dtype=np.uint64)
    lazy = spread(np.random.default_rng(7), x, moduli)
    assert np.array_equal(lazy, spread_flat(np.random.default_rng(7), x))
    assert np.array_equal(lazy % np.array(moduli, dtype=np.uint64)[:, None], x) and (lazy // np.array(moduli, dtype=np.uint64)[:, None]).max() == 3
    cube = x.reshape(3, 2, n)
    assert np.array_equal(spread(np.random.default_rng(8), cube, moduli), spread_flat(np.random.default_rng(8), x).reshape(cube.shape))
    for axis in (1, 2):
        w = np.ascontiguousarray(np.moveaxis(np.stack([cube, cube[:, ::-1]]), 1, axis))      # the prime axis of the inner product's a (1) and bhat (2)
        assert np.array_equal(spread(np.random.default_rng(9), w, moduli, axis), spread_axis(np.random.default_rng(9), w, axis))

