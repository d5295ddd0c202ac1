"""The BFV-family calls where their launches change shape: agx_ntt_basis_extend_exact and _extend_mont in both forms, agx_ntt_basis_quotient,
agx_ntt_basis_mod_down_mode (round, t = 65537), agx_ntt_plain_scale_up, _lift and _scale_down

  * past one grid-stride trip of their streaming kernels (n = 32, 140,000 frames: more work items per prime than rns_cases.TRIP), every word against the
    same call made 1,000 frames at a time;
  * in NTT form at n = 4096 on a six-prime plan of moduli 2^60 - c at the batch where the forward on the target range is the companion's (id 165), every
    word against the coefficient-form call followed by the forward of a plan over the targets (the main kernel) -- the quotient against the radix-2 twin;
  * with their scaled inverses on the big-frame routes: n = 8192 and 32768, and n = 16384 on more frames than the loop inverse's resident grid, reduced and
    lazy inputs, the scratch apart and the scratch the operand, every word against the radix-2 twin plan (the generic route).

The ranges start behind prime 0 throughout: the auxiliary prime (m, gamma) is prime 0, Q follows, B stands behind Q.  Frames at the edges of the work
decomposition are judged by the Python-integer models (bfv_conv_ref, quotient_ref, plain_ref, moddown_modes_ref) over the oracle's transforms.  Every
comparison is word for word, and every case asserts that it reached the route it names."""
import numpy as np
import pytest

import bfv_conv_ref as ref
import plain_ref as pref
import quotient_ref as qref
from gpu_util import (assert_equals_chunked_calls, companion_batches, judged_frames, loop_batch, moduli_for, oracle_tables, radix2_twin, resident_grid,
                      spread_lazy_)
from moddown_modes_ref import mod_down_mode_ntt
from q60c_skip_cases import SKIP_MAX_C
from rns_cases import TRIP
from rns_ref import oracle_forward_set, oracle_inverse_set

pytestmark = pytest.mark.gpu

COEFF, NTT = 0, 1
ROUND = 1
T = 65537
MAIN_4096, COMPANION_Q60C = 93, 165


def _u64(rows):
    return np.array(rows, dtype=np.uint64)


def _plan(agx, orc, n, moduli):
    """a plan over `moduli` with the oracle's (least) roots, which psi() reports: radix2_twin and a plan over a range of them have the same tables"""
    return agx.Plan(n, list(moduli), psi=[oracle_tables(orc, n, q)[1] for q in moduli])


class _Calls:
    """The handles of one plan for m = plan prime `aux`, Q = primes [q_first, q_first + L), B = primes [b_first, b_first + K) and the plaintext modulus T,
    and per call name its operands, the call itself and the model.  Operands are [slabs][frames][n] int64 tensors, one list for the inputs and one for the
    outputs; a slab is under a modulus, or holds any 64-bit words (None)."""

    def __init__(self, orc, dev, plan, aux, Q, B):
        self.orc, self.dev, self.plan, self.n = orc, dev, plan, plan.n
        (qf, L), (bf, K) = Q, B
        assert aux == 0 and qf >= 1 and bf >= 1, "every range starts behind prime 0"
        mod = plan.moduli
        self.Q, self.B, self.m = tuple(mod[qf:qf + L]), tuple(mod[bf:bf + K]), mod[aux]
        self.q_first, self.L, self.K = qf, L, K
        self.aux = plan.basis_aux(bf, K, qf, L, aux)            # sources B, targets Q
        self.quot = plan.basis_quotient(bf, K, qf, L, aux, T)
        self.down = plan.basis(bf, K, qf, L, T)
        self.plain = plan.plain(qf, L, aux, T)                  # gamma = m
        self.inputs = {"exact": (self.B, (self.m,)), "mont": (self.B,), "quotient": (self.Q + self.B + (self.m,),), "mod_down": (self.Q, self.B),
                       "up": ((None,),), "lift": ((None,),), "down": (self.Q,)}

    def close(self):
        for h in (self.aux, self.quot, self.down, self.plain):
            h.close()

    def out_slabs(self, name):
        return 1 if name == "down" else self.L

    def operands(self, name, batch, seed, lazy=True):
        """the inputs of `name` on the device: residues below their modulus, spread over [0, 4q) when lazy (the same residues for the same seed)"""
        torch, dev, n = self.dev.torch, self.dev, self.n
        g = torch.Generator(device=dev.device)
        g.manual_seed(seed)
        out = []
        for k, mods in enumerate(self.inputs[name]):
            v = dev.empty(len(mods) * batch * n).view(len(mods), batch, n)
            for i, q in enumerate(mods):
                draw = lambda hi: torch.randint(0, hi, (batch, n), generator=g, device=dev.device, dtype=torch.int64)      # noqa: E731
                v[i] = (draw(1 << 32) << 32) | draw(1 << 32) if q is None else draw(int(q))
            if lazy and mods[0] is not None:
                spread_lazy_(torch, v, mods, seed + 1 + k)
            out.append(v)
        return out

    def outputs(self, name, batch):
        return [self.dev.torch.full((self.out_slabs(name), batch, self.n), -1, dtype=self.dev.torch.int64, device=self.dev.device)]

    def run(self, name, ins, outs, frames, form=NTT, in_place=False):
        """the call on dense operands of `frames` frames; in_place: the scratch is the operand (which is consumed)"""
        st, p, o = self.dev.stream, [v.data_ptr() for v in ins], outs[0].data_ptr()
        if name == "exact":
            self.aux.extend_exact(p[0], p[1], o, frames, form, st)
        elif name == "mont":
            self.aux.extend_mont(p[0], o, frames, form, st)
        elif name in ("up", "lift"):
            (self.plain.scale_up if name == "up" else self.plain.lift)(p[0], o, frames, form, st)
        elif name == "quotient":
            scratch = ins[0] if in_place else self.dev.empty(ins[0].numel())
            self.quot.quotient(p[0], o, scratch.data_ptr(), frames, st)
        elif name == "mod_down":
            scratch = ins[1] if in_place else self.dev.empty(ins[1].numel())
            self.down.mod_down(p[0], p[1], o, scratch.data_ptr(), frames, st, ROUND)
        else:
            scratch = ins[0] if in_place else self.dev.empty(ins[0].numel())
            self.plain.scale_down(p[0], o, scratch.data_ptr(), frames, st)

    def model(self, name, h, form=NTT):
        """the words of the call on host copies h ([slabs][count] uint64 each) of its inputs, from Python integers over the oracle's transforms"""
        orc, n, Q, B, m = self.orc, self.n, self.Q, self.B, self.m
        if name in ("exact", "mont", "up", "lift"):
            if name == "exact":
                coeff = ref.extend_exact(h[0].tolist(), h[1][0].tolist(), B, Q, m)
            elif name == "mont":
                coeff = ref.extend_mont(h[0].tolist(), B, Q, m)
            else:
                coeff = (pref.scale_up if name == "up" else pref.lift)(h[0][0].tolist(), Q, T)
            return _u64(coeff) if form == COEFF else oracle_forward_set(orc, n, Q, _u64(coeff))
        if name == "quotient":
            rows = oracle_inverse_set(orc, n, Q + B + (m,), h[0]).tolist()
            return oracle_forward_set(orc, n, Q, _u64(qref.quotient(rows, Q, B, m, T)))
        if name == "mod_down":
            return mod_down_mode_ntt(orc, n, h[0], h[1], B, Q, T, ROUND)
        return _u64([pref.scale_down(oracle_inverse_set(orc, n, Q, h[0]).tolist(), Q, m, T)])

    def wanted(self, name, ins, frames, form=NTT):
        """the model's words for the listed frames of the inputs, [out slabs][len(frames)][n]"""
        idx = self.dev.torch.tensor(frames, device=self.dev.device)
        h = [self.dev.to_host(v[:, idx].contiguous().view(-1)).reshape(v.shape[0], -1) for v in ins]
        return self.model(name, h, form).reshape(self.out_slabs(name), len(frames), self.n)

    def judge(self, out, want, frames, what):
        idx = self.dev.torch.tensor(frames, device=self.dev.device)
        got = self.dev.to_host(out[:, idx].contiguous().view(-1)).reshape(want.shape)
        bad = [(j, frames[f]) for j in range(want.shape[0]) for f in range(len(frames)) if not np.array_equal(got[j, f], want[j, f])]
        assert not bad, (what, "(slab, frame) differ from the model", bad[:8])


# ---- past one grid-stride trip ---------------------------------------------------------------------------------------------------------
TRIP_CASES = [("exact", COEFF), ("exact", NTT), ("mont", COEFF), ("mont", NTT), ("quotient", NTT), ("mod_down", NTT), ("up", COEFF), ("up", NTT),
              ("lift", COEFF), ("lift", NTT), ("down", NTT)]


@pytest.mark.parametrize("name,form", TRIP_CASES, ids=[f"{name}-{'ntt' if form else 'coeff'}" for name, form in TRIP_CASES])
def test_past_one_grid_stride_trip(agx, orc, dev, name, form):
    """n = 32, 140,000 frames, five 60-bit primes, S = K = L = 2: more work items per prime than one trip of the streaming kernels' largest grid.  Every
    word of the large call equals the same call made 1,000 frames at a time (125 workgroups' worth per prime: one step of any grid that size or larger);
    frames across the whole range, the ends included, equal the model"""
    torch = dev.torch
    n, batch, chunk = 32, 140000, 1000
    assert batch * n > TRIP and chunk * n * 5 < TRIP
    plan = _plan(agx, orc, n, moduli_for(orc.find_prime, n, [60] * 5))
    calls = _Calls(orc, dev, plan, 0, (1, 2), (3, 2))
    ins, outs = calls.operands(name, batch, 32 + len(name) + form), calls.outputs(name, batch)
    keep = [v.clone() for v in ins]
    calls.run(name, ins, outs, batch, form)
    dev.sync()
    assert all(torch.equal(a, b) for a, b in zip(ins, keep)), (name, form, "an input changed")
    assert_equals_chunked_calls(torch, lambda i, o, frames: calls.run(name, i, o, frames, form), ins, outs, batch, chunk)
    frames = judged_frames(batch, 48, extra=range(0, batch, 4999))
    calls.judge(outs[0], calls.wanted(name, ins, frames, form), frames, (name, form))
    calls.close()
    plan.close()


# ---- NTT form on the forward companion -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exact", "mont", "up", "lift", "quotient"])
def test_ntt_form_on_the_forward_companion_of_4096(agx, orc, dev, name):
    """the library's six largest 60-bit primes (all 2^60 - c within the skip form's class), Q = primes 1 .. 3, B = primes 4, 5, the batch b_hi at which a
    forward of the plan -- and so the forward on Q behind the coefficient-form kernel -- is the companion's.  Every word equals the coefficient-form call
    followed by the forward of a plan over Q, which is below its own threshold and runs the main kernel; the quotient, which has no coefficient form,
    equals the same call under the radix-2 twin plan.  The edge frames equal the model"""
    torch = dev.torch
    n, st = 4096, dev.stream
    moduli = tuple(agx.find_primes(60, n, 6))
    assert all(0 < (1 << 60) - q <= SKIP_MAX_C for q in moduli)
    plan = _plan(agx, orc, n, moduli)
    _, batch = companion_batches(plan, MAIN_4096, COMPANION_Q60C)
    assert plan.forward_kernel(batch) == COMPANION_Q60C
    calls = _Calls(orc, dev, plan, 0, (1, 3), (4, 2))
    ins, outs = calls.operands(name, batch, 4096 + len(name)), calls.outputs(name, batch)
    keep = [v.clone() for v in ins]
    calls.run(name, ins, outs, batch, NTT)
    dev.sync()
    assert all(torch.equal(a, b) for a, b in zip(ins, keep)), (name, "an input changed")
    if name == "quotient":
        twin = radix2_twin(agx, plan)
        assert twin.forward_kernel(batch) == -1
        other = _Calls(orc, dev, twin, 0, (1, 3), (4, 2))
        want = other.outputs(name, batch)
        other.run(name, ins, want, batch, NTT)
        dev.sync()
        assert torch.equal(outs[0], want[0]), (name, "differs from the same call under the radix-2 twin plan")
        other.close()
        twin.close()
    else:
        sub = _plan(agx, orc, n, calls.Q)
        assert sub.forward_kernel(batch) == MAIN_4096 and all(sub.psi(k) == plan.psi(calls.q_first + k) for k in range(calls.L))
        want = calls.outputs(name, batch)
        calls.run(name, ins, want, batch, COEFF)
        sub.forward(want[0].data_ptr(), want[0].data_ptr(), batch, st)
        dev.sync()
        assert torch.equal(outs[0], want[0]), (name, "differs from the coefficient form followed by the forward of a plan over Q")
        sub.close()
    frames = judged_frames(batch, 6)
    calls.judge(outs[0], calls.wanted(name, ins, frames, NTT), frames, name)
    calls.close()
    plan.close()


# ---- scaled inverses on the big-frame routes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quotient", "down", "mod_down"])
@pytest.mark.parametrize("n", [8192, 16384, 32768])
def test_scaled_inverses_on_the_big_frame_routes(agx, orc, dev, n, name):
    """four 60-bit primes, Q = prime 1, B = primes 2, 3: the calls whose inverse runs with replaced last-stage constants on a range of the plan's
    primes.  Batch 2 at n = 8192 and 32768; at n = 16384 more frames than the loop inverse's resident grid, a ragged last round.  Reduced and lazy
    inputs, the scratch apart (inputs unchanged) and the scratch the operand: every word equals the radix-2 twin plan's, which takes the generic route;
    the first, the last and the frames on both sides of the resident grid equal the model"""
    torch = dev.torch
    plan = _plan(agx, orc, n, moduli_for(orc.find_prime, n, [60] * 4))
    twin = radix2_twin(agx, plan)
    batch, resident = 2, resident_grid(torch, n)
    if n == 16384:
        batch = loop_batch(torch, n)
        assert batch > resident and batch % resident != 0, (batch, resident)
    assert plan.forward_kernel(batch) != -1 and twin.forward_kernel(batch) == -1
    calls, other = _Calls(orc, dev, plan, 0, (1, 1), (2, 2)), _Calls(orc, dev, twin, 0, (1, 1), (2, 2))
    assert calls.down.mod_down_launches() == 2 and other.down.mod_down_launches() > 2, "the plan must take the two-launch ModDown, its twin the generic route"
    frames = sorted({f for f in (0, 1, batch - 2, batch - 1) + ((resident - 1, resident) if n == 16384 else ()) if 0 <= f < batch})
    seed = n + len(name)
    want_model = calls.wanted(name, calls.operands(name, batch, seed, lazy=False), frames)
    for lazy in (False, True):
        keep = calls.operands(name, batch, seed, lazy)
        want = other.outputs(name, batch)
        other.run(name, [v.clone() for v in keep], want, batch)
        for in_place in (False, True):
            what = (n, name, "lazy" if lazy else "reduced", "scratch = operand" if in_place else "scratch apart")
            ins, outs = [v.clone() for v in keep], calls.outputs(name, batch)
            calls.run(name, ins, outs, batch, in_place=in_place)
            dev.sync()
            assert torch.equal(outs[0], want[0]), (what, "differs from the radix-2 twin plan")
            assert in_place or all(torch.equal(a, b) for a, b in zip(ins, keep)), (what, "an input changed")
            calls.judge(outs[0], want_model, frames, what)
    calls.close(), other.close()
    twin.close(), plan.close()
