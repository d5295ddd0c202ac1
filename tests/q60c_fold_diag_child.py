"""Child process of tests/test_gpu_fwd_q60c_fold.py: runs with AGX_NTT_LIB = lib/libagxntt_diag.so, which holds both forward kernels for moduli
2^60 - c in the 128-thread shape -- the two-twiddle butterfly (registry id 165) and the quotient-estimate butterfly it replaced (A/B twin, id 167) --
and checks that the two ids given on the command line write identical fully reduced outputs (the oracle's) for the same 5 frames per prime: the two
boundary primes of tests/golden/q60c_boundary.json and one benchmark prime.  Prints FOLD AB OK on success."""
import json
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

assert agx.LIB_PATH.endswith("libagxntt_diag.so"), agx.LIB_PATH
old_id, new_id = int(sys.argv[1]), int(sys.argv[2])
orc.build()
dev = DeviceHelper(torch)
n, batch = 4096, 5

with open(os.path.join(ROOT, "tests", "golden", "q60c_boundary.json")) as f:
    moduli = [c["q"] for c in json.load(f)["cases"]] + [agx.find_primes(60, n, 2)[1]]
plan, tabs = plan_for_moduli(agx, orc, n, moduli, inverse=False)
rng = np.random.default_rng(167)
frames = []
for q, *_ in tabs:      # per prime: below q, [0,4q), all 4q - 1, all zero, [3q,4q)
    frames.append(np.concatenate([rand_coeffs(rng, n, q), rand_coeffs(rng, n, q, hi_mult=4), np.full(n, 4 * q - 1, dtype=np.uint64),
                                  np.zeros(n, dtype=np.uint64), rand_coeffs(rng, n, q) + np.uint64(3 * q)]))
x = np.concatenate(frames)
want = oracle_forward_rns(orc, x, tabs, n)
got = {}
for config in (old_id, new_id):
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)
    assert plan.forward_kernel(batch) == config
    d = dev.to_device(x)
    plan.forward(d.data_ptr(), d.data_ptr(), batch, dev.stream)
    got[config] = dev.to_host(d)
plan.close()
assert np.array_equal(got[old_id], got[new_id]), "the two kernels' reduced outputs differ"
assert np.array_equal(got[new_id], want), "reduced outputs differ from the oracle's"
print("FOLD AB OK")
