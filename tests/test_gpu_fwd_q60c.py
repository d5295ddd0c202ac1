"""The forward kernel specialised for moduli q = 2^60 - c, 0 < c < 2^28 (registry id 165: the n = 4096 streamed 128-thread kernel with
sign-bit conditional subtracts and the final reduction by the top four bits; its 512-thread A/B twin 166 lives in lib/libagxntt_diag.so).
A plan takes it only when EVERY modulus is of that class (arithmetic level 3); fully reduced outputs depend on (x, q, psi) alone, so every
result is compared bit for bit with the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import oracle_tables, plan_for_moduli, rand_coeffs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
Q60C_ID, GENERAL_COMPANION_ID, MAIN_ID, TWIN_ID = 165, 159, 93, 166
BIG = 4096 + 1      # frames per prime: with any number of primes past the companion's 4,096-frame threshold, and an odd tail
PERIOD = 7          # the big batch repeats PERIOD distinct frames (odd: every frame meets workgroups of every parity)


def _input_kinds(rng, q, frames):
    """the four input fills of `frames` frames each: below q, all q - 1, all zero, and [3q, 4q) -- the top of the legal input range"""
    return {
        "below q": rand_coeffs(rng, frames * N, q),
        "all q-1": np.full(frames * N, q - 1, dtype=np.uint64),
        "all zero": np.zeros(frames * N, dtype=np.uint64),
        "[3q,4q)": rand_coeffs(rng, frames * N, q) + np.uint64(3 * q),
    }


@pytest.fixture(scope="module")
def bench_case(agx, orc):
    """the four benchmark primes, the frames every test of this module transforms, and the oracle's transform of them, computed once:
    per prime 3 frames of each input kind (batches 1 and 3), and PERIOD base frames for the big batch (3 below q, q - 1, zero, 2 in [3q,4q))"""
    tabs = [oracle_tables(orc, N, q) for q in agx.find_primes(60, N, 4)]
    rng = np.random.default_rng(165)
    small = [_input_kinds(rng, t[0], 3) for t in tabs]
    base = []
    for t, kinds in zip(tabs, small):
        extra = _input_kinds(rng, t[0], 2)
        base.append(np.concatenate([kinds["below q"], kinds["all q-1"][:N], kinds["all zero"][:N], extra["[3q,4q)"]]))
    fwd = lambda x, t: orc.forward(x, t[0], t[2], t[3], N)      # noqa: E731
    small_want = [{k: fwd(v, t) for k, v in kinds.items()} for t, kinds in zip(tabs, small)]
    base_want = [fwd(b, t) for b, t in zip(base, tabs)]
    for a in base + base_want + [v for d in small + small_want for v in d.values()]:
        a.setflags(write=False)
    return {"tabs": tabs, "small": small, "small_want": small_want, "base": base, "base_want": base_want}


def _small(case, key, kind, batch):
    """[prime][batch][n] flat: the first `batch` frames of the given kind under every prime"""
    return np.concatenate([d[kind][:batch * N] for d in case[key]])


def _tiled(dev, frames):
    """[prime][PERIOD][n] on the host -> [prime][BIG][n] on the device, frame f = base frame f % PERIOD"""
    torch = dev.torch
    t = dev.to_device(np.concatenate(frames)).view(len(frames), PERIOD, N)
    idx = torch.arange(BIG, device=dev.device) % PERIOD
    return t[:, idx, :].contiguous().view(-1)


def _check_lazy(got, want, tabs, batch, where):
    for p, t in enumerate(tabs):
        sl = slice(p * batch * N, (p + 1) * batch * N)
        assert (got[sl] < np.uint64(4 * t[0])).all(), (where, p, "a lazy output at or above 4q")
        assert np.array_equal(got[sl] % np.uint64(t[0]), want[sl]), (where, p, "lazy outputs not congruent to the oracle's")


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", [False, True], ids=["reduced", "lazy"])
def test_specialised_path_small_batches(agx, orc, dev, bench_case, lazy):
    """cases A and B at 1 and 3 frames per prime: the plan's own choice for launches this small is the 512-thread kernel (id 93), so the specialised
    kernel is selected explicitly -- it must be legal for these moduli"""
    tabs = bench_case["tabs"]
    plan, _ = plan_for_moduli(agx, orc, N, [t[0] for t in tabs], inverse=False)
    assert plan.forward_kernel(1) == MAIN_ID and plan.forward_kernel(3) == MAIN_ID
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + Q60C_ID)
    for batch in (1, 3):
        assert plan.forward_kernel(batch) == Q60C_ID
        for kind in bench_case["small"][0]:
            x, want = _small(bench_case, "small", kind, batch), _small(bench_case, "small_want", kind, batch)
            d = dev.to_device(x)
            (plan.forward_lazy if lazy else plan.forward)(d.data_ptr(), d.data_ptr(), batch, dev.stream)
            got = dev.to_host(d)
            if lazy:
                _check_lazy(got, want, tabs, batch, (batch, kind))
            else:
                assert np.array_equal(got, want), (batch, kind)
    plan.close()


@pytest.mark.gpu
def test_specialised_path_is_the_default_past_the_companion_threshold(agx, orc, dev, bench_case):
    """cases A and B at 4,096 + 1 frames per prime: the plan itself sends the launch to id 165; every frame, reduced and lazy, on the device"""
    torch = dev.torch
    tabs = bench_case["tabs"]
    plan, _ = plan_for_moduli(agx, orc, N, [t[0] for t in tabs], inverse=False)
    assert plan.forward_kernel(BIG) == Q60C_ID
    d_x, d_want = _tiled(dev, bench_case["base"]), _tiled(dev, bench_case["base_want"])
    d_y = dev.empty(d_x.numel())
    plan.forward(d_x.data_ptr(), d_y.data_ptr(), BIG, dev.stream)
    dev.sync()
    bad = (d_y != d_want).nonzero().flatten()[:4].tolist()
    assert not bad, ("reduced outputs differ from the oracle's at", bad)
    d_y.zero_()
    plan.forward_lazy(d_x.data_ptr(), d_y.data_ptr(), BIG, dev.stream)
    dev.sync()
    y = d_y.view(len(tabs), -1)
    for p, t in enumerate(tabs):
        # words are below 4q < 2^62, so int64 arithmetic is exact
        assert bool((y[p] >= 0).all()) and bool((y[p] < 4 * t[0]).all()), (p, "a lazy output at or above 4q")
        assert torch.equal(y[p] % t[0], d_want.view(len(tabs), -1)[p]), (p, "lazy outputs not congruent to the oracle's")
    plan.close()


def _upward_60bit_prime(orc):
    q = (1 << 59) + 1
    while not orc.is_prime(q):
        q += 2 * N
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("outsider", ["59-bit", "60-bit from 2^59 upward"])
def test_one_modulus_outside_the_class_falls_back(agx, orc, dev, outsider):
    """case C: one prime outside the class (a 59-bit prime; the first 60-bit NTT prime above 2^59, whose c is nearly 2^59) sends the whole plan to the
    general kernels -- id 159 past the threshold, id 93 below it -- and id 165 refuses the plan"""
    q_out = orc.find_prime(59, N, 0) if outsider == "59-bit" else _upward_60bit_prime(orc)
    assert q_out < (1 << 60) - (1 << 28)
    plan, tabs = plan_for_moduli(agx, orc, N, [agx.find_primes(60, N, 1)[0], q_out], inverse=False)
    batch = 2048      # x 2 primes: exactly on the companion's threshold
    assert plan.forward_kernel(batch) == GENERAL_COMPANION_ID and plan.forward_kernel(3) == MAIN_ID
    rng = np.random.default_rng(59)
    base = [rand_coeffs(rng, PERIOD * N, t[0], hi_mult=4) for t in tabs]
    want = np.concatenate([np.tile(orc.forward(b, t[0], t[2], t[3], N).reshape(PERIOD, N), (batch // PERIOD + 1, 1))[:batch].reshape(-1) for b, t in zip(base, tabs)])
    x = np.concatenate([np.tile(b.reshape(PERIOD, N), (batch // PERIOD + 1, 1))[:batch].reshape(-1) for b in base])
    d = dev.to_device(x)
    plan.forward(d.data_ptr(), d.data_ptr(), batch, dev.stream)
    assert np.array_equal(dev.to_host(d), want)
    d3 = dev.to_device(np.concatenate([b[:3 * N] for b in base]))
    plan.forward(d3.data_ptr(), d3.data_ptr(), 3, dev.stream)
    assert np.array_equal(dev.to_host(d3), np.concatenate([want[p * batch * N:p * batch * N + 3 * N] for p in range(2)]))
    with pytest.raises(agx.AgxError) as ei:
        plan.set_variant(agx.VARIANT_REGBLOCK_BASE + Q60C_ID)
    assert ei.value.status == 2
    plan.close()


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "q60c_boundary.json")) as f:
        g = json.load(f)
    assert g["n"] == N
    return g["cases"]


def test_golden_boundary_primes_are_the_boundary(orc):
    """the fixture's moduli are the admitted 60-bit primes = 1 (mod 8192) with the smallest and the largest c < 2^28, and its outputs the oracle's"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_q60c_boundary import boundary_primes

    cases = _golden()
    assert [c["q"] for c in cases] == list(boundary_primes())
    for c in cases:
        q = c["q"]
        assert c["c"] == (1 << 60) - q and 0 < c["c"] < (1 << 28) and q % (2 * N) == 1 and c["psi"] == orc.min_root(q, N)
        tw, pre = orc.make_tables(q, c["psi"], N)
        want = np.array([int(h, 16) for h in c["forward_hex"]], dtype=np.uint64)
        assert np.array_equal(orc.forward(orc.fill_splitmix(N, c["seed"], q), q, tw, pre, N), want)


@pytest.mark.gpu
def test_boundary_values_of_c(agx, orc, dev):
    """case D: one plan over the smallest and the largest c; one frame each against the committed oracle outputs, then 3 frames of every input kind"""
    cases = _golden()
    plan, tabs = plan_for_moduli(agx, orc, N, [c["q"] for c in cases], inverse=False)
    assert [t[1] for t in tabs] == [c["psi"] for c in cases]
    assert plan.forward_kernel(BIG) == Q60C_ID
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + Q60C_ID)
    x = np.concatenate([orc.fill_splitmix(N, c["seed"], c["q"]) for c in cases])
    want = np.array([int(h, 16) for c in cases for h in c["forward_hex"]], dtype=np.uint64)
    d = dev.to_device(x)
    plan.forward(d.data_ptr(), d.data_ptr(), 1, dev.stream)
    assert np.array_equal(dev.to_host(d), want)
    rng = np.random.default_rng(28)
    kinds = [_input_kinds(rng, t[0], 3) for t in tabs]
    for kind in kinds[0]:
        x = np.concatenate([k[kind] for k in kinds])
        want = np.concatenate([orc.forward(k[kind], t[0], t[2], t[3], N) for k, t in zip(kinds, tabs)])
        for lazy in (False, True):
            d = dev.to_device(x)
            (plan.forward_lazy if lazy else plan.forward)(d.data_ptr(), d.data_ptr(), 3, dev.stream)
            got = dev.to_host(d)
            if lazy:
                _check_lazy(got, want, tabs, 3, kind)
            else:
                assert np.array_equal(got, want), kind
    plan.close()


def test_top_bits_fold_range_and_congruence():
    """case E: the final reduction of csrc/modarith.hpp (reduce_final_q60c) restated in Python integers: v = k 2^60 + r -> r + k c, which must be
    congruent to v and below 2q at the corners of the range, for both boundary values of c; one conditional subtract then lands in [0,q)"""
    for case in _golden():
        q, c = case["q"], case["c"]
        assert q == (1 << 60) - c
        for v in (0, q - 1, q, 8 * q - 1, 8 * q, 16 * q - 1, 16 * q + 8 * c - 1, (1 << 64) - 1):      # the last two: the sign-bit schedule's slack, any 64-bit word
            assert v < 1 << 64
            k, r = v >> 60, v & ((1 << 60) - 1)
            t = r + k * c
            assert k <= 15 and k * c < 1 << 32 and t < 2 * q and t % q == v % q, (q, v)
            assert (t - q if t >= q else t) == v % q
        # the mid-transform subtract (csub_8q_q60c): sign bit set -> x - 8q = (x - 2^63) + 8c, else x < 2^63 = 8q + 8c
        assert (1 << 63) == 8 * q + 8 * c and 8 * c < 1 << 31 and 16 * q + 8 * c < 1 << 64
        for x in (0, 8 * q - 1, 8 * q, (1 << 63) - 1, 1 << 63, 16 * q - 1, 16 * q + 8 * c - 1):
            tx = (x & ((1 << 63) - 1)) + (x >> 63) * 8 * c
            assert tx % q == x % q and tx < 1 << 63, (q, x)


@pytest.mark.gpu
def test_diag_twin_in_the_512_thread_shape(agx):
    """the A/B twin (id 166: id 93's forward kernel with the same arithmetic) is only in lib/libagxntt_diag.so; a process binds one library, so it is
    checked in a child bound to that one (tests/q60c_diag_child.py)"""
    if not os.path.exists(agx.DIAG_LIB_PATH):
        agx.build_diag()
    env = dict(os.environ, AGX_NTT_LIB=agx.DIAG_LIB_PATH)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "q60c_diag_child.py"), str(TWIN_ID)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Q60C TWIN OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
