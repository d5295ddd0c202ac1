"""bench.py's plain run and --dump-outputs: the result line of a plain run holds the headline and nothing that --full adds, and the
dumped arrays are the last timed step's output -- the same in every run with the same arguments, bit-exact against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, PRIMES, BATCH, SLABS = 4096, 4, 64, 4
WARMUP, STEPS = 1, 2
LAST = (WARMUP + STEPS - 1) % SLABS      # the slab the last timed step transformed (step i uses slab i mod 4)


def _bench(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--batch", str(BATCH),
                        "--ramp-seconds", "0.1", "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    hi, lo = np.load(out_dir / "forward_hi32.npy"), np.load(out_dir / "forward_lo32.npy")
    assert hi.dtype == lo.dtype == np.float64 and hi.shape == lo.shape == (PRIMES * BATCH, N)
    return json.loads(lines[0]), (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)


def _expected(agx, orc, dev, first_poly):
    """forward NTT of the synthetic slab that starts at polynomial first_poly: WARMUP + STEPS <= 4 steps each transform a
    different slab once, so the last step's output is one forward of slab LAST's synthetic data"""
    qs = agx.find_primes(60, N, PRIMES)
    plan = agx.Plan(N, qs)
    d = dev.empty(PRIMES * BATCH * N)
    plan.fill_synthetic(d.data_ptr(), BATCH, first_poly, 42, dev.stream)
    x = dev.to_host(d).reshape(PRIMES, BATCH * N)
    want = []
    for p, q in enumerate(qs):
        tw, pre = orc.make_tables(q, plan.psi(p), N)
        want.append(orc.forward(x[p].copy(), q, tw, pre, N))
    plan.close()
    return np.concatenate(want).reshape(PRIMES * BATCH, N)


def test_bench_plain_run_dumps_the_last_steps_forward_ntt(agx, orc, dev, tmp_path):
    j, a = _bench(tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in j, key
    assert j["unit"] == "NTT/s" and j["higher_is_better"] is True and j["dtype"] == "u64" and j["steps"] == STEPS and j["ms_per_step"] > 0
    assert not {"secondary", "cpu_baseline", "power"} & set(j)      # --full only
    _, b = _bench(tmp_path / "b")
    assert np.array_equal(a, b)      # same arguments, same inputs, same outputs
    assert np.array_equal(a, _expected(agx, orc, dev, LAST * BATCH))


def test_bench_single_process_dumps_shard_0(agx, orc, dev, tmp_path):
    """--single-process --devices 0,0: two shards on one GPU; shard 0's slab k starts at polynomial 2 k B"""
    j, a = _bench(tmp_path / "g", "--single-process", "--devices", "0,0")
    assert j["steps"] == STEPS and j["ms_per_step"] > 0 and len(j["per_rank"]) == 2
    assert np.array_equal(a, _expected(agx, orc, dev, 2 * LAST * BATCH))
