"""Child process of tests/test_gpu_fwd_q60c_rare_sub.py: runs with AGX_NTT_LIB = lib/libagxntt_diag.so, which holds registry id 165 and its A/B twins
169 (the two kernels it launched before the rare last subtract and the scalar table bases), 170 and 171 (each of the two alone).  Runs the ids given on
the command line, the last being the one under test, on the frames that force the subtract (tests/q60c_rare_cases.py), on a plan for each of the two
kernels behind the ids (skip form: the benchmark's smallest c and the largest c at the limit; every stage: one c on each side of the limit), and checks
that all write identical fully reduced words, the oracle's, and identical lazy words.  Prints RARE SUB AB OK on success."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agilex_ntt_amd as agx  # noqa: E402
from gpu_util import DeviceHelper, oracle_forward_rns, plan_for_moduli  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from q60c_rare_cases import N, forced_frames, planted_frames  # noqa: E402
from q60c_skip_cases import SKIP_MAX_C, prime_above_c, prime_at_or_below_c  # noqa: E402

assert agx.LIB_PATH.endswith("libagxntt_diag.so"), agx.LIB_PATH
ids = [int(a) for a in sys.argv[1:]]
assert len(ids) >= 2
orc.build()
dev = DeviceHelper(torch)
rng = np.random.default_rng(169)
q_in, q_out = prime_at_or_below_c(orc, SKIP_MAX_C)[0], prime_above_c(orc, SKIP_MAX_C)[0]

for moduli in ([agx.find_primes(60, N, 1)[0], q_in], [q_in, q_out]):
    plan, tabs = plan_for_moduli(agx, orc, N, moduli, inverse=False)
    x = np.concatenate([np.concatenate([forced_frames(q), planted_frames(orc, rng, q, psi)[0]]) for q, psi, *_ in tabs])
    batch = x.size // (N * len(moduli))
    want = oracle_forward_rns(orc, x, tabs, N)
    got, lazy = {}, {}
    for config in ids:
        plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)
        assert plan.forward_kernel(batch) == config
        d = dev.to_device(x)
        plan.forward(d.data_ptr(), d.data_ptr(), batch, dev.stream)
        got[config] = dev.to_host(d)
        d = dev.to_device(x)
        plan.forward_lazy(d.data_ptr(), d.data_ptr(), batch, dev.stream)
        lazy[config] = dev.to_host(d)
    plan.close()
    for config in ids:
        assert np.array_equal(got[config], want), (config, moduli, "reduced outputs differ from the oracle's")
        assert np.array_equal(lazy[config], lazy[ids[-1]]), (config, moduli, "lazy words differ between the twins")

print("RARE SUB AB OK")
