"""Child process of tests/test_gpu_fwd_q60c_skip.py: runs with AGX_NTT_LIB = lib/libagxntt_diag.so, which holds registry id 165 (on a plan whose
moduli 2^60 - c all have c <= 2^27: the skip form of the two-twiddle butterfly) and its A/B twin 168, which always launches the kernel with the
sign-bit subtract on every stage.  Checks that the two ids given on the command line write identical fully reduced outputs (the oracle's) for the same
5 frames per prime: the largest c at the limit, a c near 2^26 and the benchmark's smallest c.  Prints SKIP AB OK on success."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agilex_ntt_amd as agx  # noqa: E402
from gpu_util import DeviceHelper, oracle_forward_rns, plan_for_moduli, rand_coeffs  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from q60c_skip_cases import SKIP_MAX_C, prime_at_or_below_c  # noqa: E402

assert agx.LIB_PATH.endswith("libagxntt_diag.so"), agx.LIB_PATH
twin_id, skip_id = int(sys.argv[1]), int(sys.argv[2])
orc.build()
dev = DeviceHelper(torch)
n, batch = 4096, 5

moduli = [prime_at_or_below_c(orc, SKIP_MAX_C)[0], prime_at_or_below_c(orc, 1 << 26)[0], agx.find_primes(60, n, 1)[0]]
assert len(set(moduli)) == 3 and all(0 < (1 << 60) - q <= SKIP_MAX_C for q in moduli)
plan, tabs = plan_for_moduli(agx, orc, n, moduli, inverse=False)
rng = np.random.default_rng(168)
frames = []
for q, *_ in tabs:      # per prime: below q, [0,4q), all 4q - 1, all zero, [3q,4q)
    frames.append(np.concatenate([rand_coeffs(rng, n, q), rand_coeffs(rng, n, q, hi_mult=4), np.full(n, 4 * q - 1, dtype=np.uint64),
                                  np.zeros(n, dtype=np.uint64), rand_coeffs(rng, n, q) + np.uint64(3 * q)]))
x = np.concatenate(frames)
want = oracle_forward_rns(orc, x, tabs, n)
got = {}
for config in (twin_id, skip_id):
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)
    assert plan.forward_kernel(batch) == config
    d = dev.to_device(x)
    plan.forward(d.data_ptr(), d.data_ptr(), batch, dev.stream)
    got[config] = dev.to_host(d)
plan.close()
assert np.array_equal(got[twin_id], got[skip_id]), "the two kernels' reduced outputs differ"
assert np.array_equal(got[skip_id], want), "reduced outputs differ from the oracle's"

print("SKIP AB OK")
