"""Child process of tests/test_gpu_fwd_q60c.py: runs with AGX_NTT_LIB = lib/libagxntt_diag.so and checks the registry entry given on the command
line (the 512-thread A/B twin of the forward kernel for moduli 2^60 - c) against the oracle.  Prints Q60C TWIN OK on success."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agilex_ntt_amd as agx  # noqa: E402
from gpu_util import DeviceHelper, oracle_forward_rns, plan_from_oracle_tables, rand_coeffs  # noqa: E402
from oracle import oracle as orc  # noqa: E402

assert agx.LIB_PATH.endswith("libagxntt_diag.so"), agx.LIB_PATH
config = int(sys.argv[1])
orc.build()
dev = DeviceHelper(torch)
n, batch = 4096, 3

plan, tabs = plan_from_oracle_tables(agx, orc, n, 60, 2, inverse=False)
plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)
assert plan.forward_kernel(batch) == config
rng = np.random.default_rng(config)
for hi_mult, lazy in ((1, False), (4, False), (4, True)):
    x = np.concatenate([rand_coeffs(rng, batch * n, t[0], hi_mult=hi_mult) for t in tabs])
    if hi_mult == 4:
        x[:n] = np.uint64(4 * tabs[0][0] - 1)      # one frame at the very top of the input range
    want = oracle_forward_rns(orc, x, tabs, n)
    d = dev.to_device(x)
    (plan.forward_lazy if lazy else plan.forward)(d.data_ptr(), d.data_ptr(), batch, dev.stream)
    got = dev.to_host(d)
    for p, t in enumerate(tabs):
        sl = slice(p * batch * n, (p + 1) * batch * n)
        if lazy:
            assert (got[sl] < np.uint64(4 * t[0])).all() and np.array_equal(got[sl] % np.uint64(t[0]), want[sl]), (hi_mult, p)
        else:
            assert np.array_equal(got[sl], want[sl]), (hi_mult, p)
plan.close()

# a modulus outside the class must be refused
plan, tabs = plan_from_oracle_tables(agx, orc, n, 59, 1, inverse=False)
try:
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)
    raise SystemExit(f"config {config} accepted a 59-bit modulus")
except agx.AgxError as e:
    assert e.status == 2
plan.close()
print("Q60C TWIN OK")
