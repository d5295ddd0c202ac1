"""Helpers for the GPU parity tests: torch is only the device-memory allocator here."""
import numpy as np


class DeviceHelper:
    def __init__(self, torch):
        self.torch = torch
        self.device = torch.device("cuda:0")

    def to_device(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        return self.torch.from_numpy(a.view(np.int64).copy()).to(self.device)

    def empty(self, count):
        return self.torch.empty(int(count), dtype=self.torch.int64, device=self.device)

    def to_host(self, t):
        self.torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint64).copy()

    def sync(self):
        self.torch.cuda.synchronize()

    @property
    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream


def rand_coeffs(rng, count, q, hi_mult=1):
    """uniform in [0, hi_mult*q) as uint64 (hi_mult up to 4: the lazy input range)"""
    hi = int(q) * hi_mult
    # numpy's integers() handles bounds up to 2^64 with dtype=uint64
    return rng.integers(0, hi, size=count, dtype=np.uint64)


def tables_for(orc, n, bits, count=1):
    """[(q, psi, tw, pre)] for the `count` largest primes below 2^bits"""
    out = []
    for k in range(count):
        q = orc.find_prime(bits, n, k)
        psi = orc.min_root(q, n)
        tw, pre = orc.make_tables(q, psi, n)
        out.append((q, psi, tw, pre))
    return out


def oracle_polymul(orc, a, b, q, psi, n):
    """INTT(NTT(a) o NTT(b)) through the oracle's own transforms, frame by frame (operands may be lazy: reduced first)"""
    tw, pre = orc.make_tables(q, psi, n)
    itw, _ = orc.make_inv_tables(q, psi, n)
    fa = orc.forward(a % np.uint64(q), q, tw, pre, n)
    fb = orc.forward(b % np.uint64(q), q, tw, pre, n)
    return orc.inverse(orc.pointwise(fa, fb, q), q, itw, n)


def radix2_twin(agx, plan):
    """a second plan with the same moduli and roots (so the same tables), forced onto the radix-2 LDS kernels: an independent
    kernel family for full-batch differential checks (its products take the three-launch path and need caller scratch)"""
    twin = agx.Plan(plan.n, plan.moduli, psi=[plan.psi(p) for p in range(plan.num_primes)])
    twin.set_variant(agx.VARIANT_LDS_RADIX2)
    return twin


def shift_exponents(torch, first, count, n, device):
    """j_f = (f * 2654435761) mod n for frames f = first .. first + count - 1: the monomial X^j_f of frame f"""
    f = torch.arange(first, first + count, dtype=torch.int64, device=device)
    return (f * 2654435761) % n


def fill_monomials(torch, t, primes, batch, n):
    """t ([primes][batch][n] int64 on the device): frame f of every prime = X^j_f, filled in chunks of frames"""
    v = t.view(primes, batch, n)
    step = max(1, (1 << 27) // n)
    for f0 in range(0, batch, step):
        f1 = min(batch, f0 + step)
        v[:, f0:f1].zero_()
        j = shift_exponents(torch, f0, f1 - f0, n, t.device)
        rows = torch.arange(f1 - f0, device=t.device)
        v[:, f0:f1][:, rows, j] = 1


def check_negacyclic_shifts(torch, c, b, moduli, batch, n):
    """every frame f of c ([primes][batch][n] on the device) must be X^j_f * b_f mod (X^n + 1, q_p), b in [0, q): built on the device
    with gather / where, compared with torch.equal in chunks of frames; returns a list of (prime, first bad frames) (empty = pass)"""
    primes = len(moduli)
    cv, bv = c.view(primes, batch, n), b.view(primes, batch, n)
    i = torch.arange(n, dtype=torch.int64, device=c.device)[None, :]
    step = max(1, (1 << 26) // n)
    bad = []
    for p, q in enumerate(moduli):
        for f0 in range(0, batch, step):
            f1 = min(batch, f0 + step)
            j = shift_exponents(torch, f0, f1 - f0, n, c.device)[:, None]
            v = torch.gather(bv[p, f0:f1], 1, (i - j) % n)
            want = torch.where(i < j, (int(q) - v) % int(q), v)
            got = cv[p, f0:f1]
            if not torch.equal(got, want):
                rows = (got != want).any(dim=1).nonzero().flatten()[:4]
                bad.append((p, [f0 + int(r) for r in rows]))
    return bad


def boundary_frames(batch, extra=()):
    """frames where a launch's work decomposition changes: 0, 1, the last and the first of the last partial wave (batch - 3), both
    sides of every power of two (frames per workgroup = frames per wave x waves per workgroup), both sides of multiples of 256 up to
    4096 (the loop kernels' resident grid is CUs x workgroups per CU), plus `extra`"""
    s = {0, 1, batch - 1, batch - 3}
    k = 1
    while k <= batch:
        s |= {k - 1, k}
        k *= 2
    for m in range(256, 4097, 256):
        s |= {m - 1, m}
    s |= set(extra)
    return sorted(f for f in s if 0 <= f < batch)
