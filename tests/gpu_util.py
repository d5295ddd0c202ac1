"""Shared support of the tests, written once: device memory (torch is only the allocator here), moduli / oracle tables / plans, the
oracle over dense frame sets, status_of, the one stream-capture helper, the group-of-two scaffolding, guarded arenas, whole-buffer
checkers, and the kernel registry as the tests know it.  No test module imports another test module; they import from here, and the tests of the
RNS calls from rns_ref.py (the Python-integer reference) and rns_cases.py (cases two files share) besides."""
import functools

import numpy as np
import pytest


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


# ---------------------------------------------------------------------------------------
# moduli, the oracle's tables, plans made from them
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_tables(orc, n, q):
    """(q, psi, tw, pre) for the least root of q, computed once per (n, q) and shared by every test: the arrays are read-only"""
    psi = orc.min_root(q, n)
    tw, pre = orc.make_tables(q, psi, n)
    tw.setflags(write=False)
    pre.setflags(write=False)
    return q, psi, tw, pre


def moduli_for(find_prime, n, spec):
    """spec: modulus widths in bits; the k-th use of a width takes find_prime(bits, n, k), the k-th largest prime below 2^bits.
    find_prime is the oracle's (orc.find_prime) or the library's (library_find_prime(agx))"""
    seen, out = {}, []
    for bits in spec:
        out.append(find_prime(bits, n, seen.get(bits, 0)))
        seen[bits] = seen.get(bits, 0) + 1
    return tuple(out)


def library_find_prime(agx):
    """the library's prime finder with the oracle's signature"""
    return lambda bits, n, k=0: agx.find_primes(bits, n, k + 1)[k]


def plan_for_moduli(agx, orc, n, moduli, inverse=True):
    """(plan, tabs): a plan created from the oracle's own tables for `moduli`, tabs = [(q, psi, tw, pre)]"""
    tabs = [oracle_tables(orc, n, q) for q in moduli]
    tables = [np.stack([t[2] for t in tabs]), np.stack([t[3] for t in tabs])]
    if inverse:
        inv = [orc.make_inv_tables(t[0], t[1], n) for t in tabs]
        tables += [np.stack([i[0] for i in inv]), np.stack([i[1] for i in inv])]
    return agx.Plan(n, list(moduli), tables=tuple(tables)), tabs


def tables_for(orc, n, bits, count=1):
    """[(q, psi, tw, pre)] for the `count` largest primes below 2^bits"""
    return [oracle_tables(orc, n, q) for q in moduli_for(orc.find_prime, n, [bits] * count)]


def plan_from_oracle_tables(agx, orc, n, bits, count, inverse=True):
    """(plan, tabs) for the `count` largest primes below 2^bits, the plan created from the oracle's own tables"""
    return plan_for_moduli(agx, orc, n, moduli_for(orc.find_prime, n, [bits] * count), inverse)


def oracle_forward_rns(orc, x, tabs, n):
    """the oracle's forward of a dense [prime][...][n] set x (any shape of that size) under tabs = [(q, psi, tw, pre)], flat"""
    x = np.asarray(x).reshape(len(tabs), -1)
    return np.concatenate([orc.forward(np.ascontiguousarray(x[p]), q, tw, pre, n) for p, (q, _, tw, pre) in enumerate(tabs)])


def status_of(agx, fn, *args):
    """0 when fn(*args) returns, the status of the AgxError it raises otherwise"""
    try:
        fn(*args)
        return 0
    except agx.AgxError as e:
        return e.status


def capture(dev, warm_up, body):
    """A HIP graph of the launches body(stream) makes.  warm_up(stream) runs first, on the same side stream and OUTSIDE the capture
    (first launches may load code objects or allocate, which a capture cannot record), and is synchronised; both take the raw stream
    handle.  Everything is recorded on exactly one stream: captured graphs here must have no parallel branches, because the runtime
    replays the branches of a graph on separate hardware queues and has crashed doing so where a process owns few of them.  The device
    is synchronised in front, the side stream waits for the current one before and the current one for the side stream after, so the
    caller's buffers are ready when the warm-up reads them and the graph is ready to replay when this returns."""
    torch = dev.torch
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    dev.sync()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm_up(side.cuda_stream)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            body(torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    return graph


def group_of_two(agx, orc, n, moduli, frames):
    """(group, plan, batches): a DeviceGroup on devices [0, 0] and the single Plan with the same moduli and (least) roots, and the
    frames each of the two shards gets when `frames` (odd) are dealt to them"""
    psi = [oracle_tables(orc, n, q)[1] for q in moduli]
    grp = agx.DeviceGroup([0, 0], n, list(moduli), psi=psi)
    plan = agx.Plan(n, list(moduli), psi=psi)
    batches = [agx.shard_block(frames, 2, i)[1] for i in range(2)]
    assert sum(batches) == frames and batches[0] != batches[1]
    return grp, plan, batches


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


# ---------------------------------------------------------------------------------------
# guarded arenas: where the words of a call live, and what a call must leave alone
# ---------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def splitmix64(i):
    """the splitmix64 output function of the uint64 indices i (numpy array), wrapping arithmetic"""
    with np.errstate(over="ignore"):
        z = (np.asarray(i, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)) & np.uint64(_M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def canary(first, count):
    """canary[i] = splitmix64(i) | 2^63 for i = first .. first + count - 1.  Bit 63 keeps every word at or above 2^62, the bound of
    the moduli, so no residue equals it; the words differ at every index, so canary data copied to another place is caught too"""
    return splitmix64(np.arange(first, first + count, dtype=np.uint64)) | np.uint64(1 << 63)


class Layout:
    """where the frames of a [prime][batch][n] operand live: frame (p, b) starts at element offset + p * prime_stride + b * poly_stride of
    the payload of an arena (the base pointer of the call is the payload's element `offset`)"""

    def __init__(self, n, primes, batch, prime_stride=None, poly_stride=None, offset=0):
        self.n, self.primes, self.batch = int(n), int(primes), int(batch)
        self.poly_stride = self.n if poly_stride is None else int(poly_stride)
        self.prime_stride = self.batch * self.n if prime_stride is None else int(prime_stride)
        self.offset = int(offset)

    def at(self, offset):
        return Layout(self.n, self.primes, self.batch, self.prime_stride, self.poly_stride, offset)

    def starts(self):
        """payload index of the first word of every frame, [primes][batch]"""
        p = np.arange(self.primes, dtype=np.int64)[:, None] * self.prime_stride
        b = np.arange(self.batch, dtype=np.int64)[None, :] * self.poly_stride
        return self.offset + p + b

    def span(self):
        """payload words from index 0 to the end of the last frame"""
        return int(self.starts().max()) + self.n

    def index(self):
        """payload index of every frame word, [primes][batch][n]"""
        return self.starts()[:, :, None] + np.arange(self.n, dtype=np.int64)[None, None, :]

    def __repr__(self):
        return (f"Layout(n={self.n}, primes={self.primes}, batch={self.batch}, prime_stride={self.prime_stride}, "
                f"poly_stride={self.poly_stride}, offset={self.offset})")


def scatter_frames(words, base, layout, frames):
    """frames ([primes][batch][n], any shape of that size) -> words[base + layout.index()]"""
    words[base + layout.index().reshape(-1)] = np.asarray(frames, dtype=np.uint64).reshape(-1)


def gather_frames(words, base, layout):
    """the frames of `layout` out of `words`, flat [primes][batch][n]"""
    return words[base + layout.index().reshape(-1)].copy()


def arena_faults(image, band, placed, limit=4):
    """Compare an arena image (uint64 words: band | payload | band) with what it must hold: the canary at every word that belongs to no
    frame, and, for every (layout, frames) of `placed` whose frames are not None, those frames.  Frames given as None are the call's
    outputs: their words are not judged here.  Returns up to `limit` faults, lowest index first, each a dict with
      index  -- payload index of the word (negative: leading band),   got / want -- the word found and the word expected,
      prime, frame, rel -- the nearest frame and the word's position relative to its first word (rel < 0: before it, rel >= n: behind it)"""
    image = np.asarray(image, dtype=np.uint64)
    want = canary(0, image.size)
    judged = np.ones(image.size, dtype=bool)
    firsts, owners = [], []
    n = None
    for layout, frames in placed:
        n = layout.n
        idx = band + layout.index().reshape(-1)
        if frames is None:
            judged[idx] = False
        else:
            want[idx] = np.asarray(frames, dtype=np.uint64).reshape(-1)
        st = layout.starts()
        firsts.append(st.reshape(-1))
        owners += [(p, b) for p in range(layout.primes) for b in range(layout.batch)]
    bad = np.flatnonzero(judged & (image != want))[:limit]
    if bad.size == 0:
        return []
    firsts = np.concatenate(firsts)
    order = np.argsort(firsts, kind="stable")
    out = []
    for i in bad:
        pay = int(i) - band
        k = int(np.searchsorted(firsts[order], pay, side="right")) - 1        # last frame that starts at or before the word
        cands = [c for c in (k, k + 1) if 0 <= c < order.size]

        def distance(c):
            s = int(firsts[order[c]])
            return 0 if s <= pay < s + n else (s - pay if pay < s else pay - (s + n - 1))

        c = min(cands, key=distance)
        p, b = owners[int(order[c])]
        out.append({"index": pay, "got": int(image[i]), "want": int(want[i]), "prime": p, "frame": b, "rel": pay - int(firsts[order[c]])})
    return out


class GuardedArena:
    """One allocation = leading band | payload | trailing band, every word pre-filled with canary(index); the bands hold at least
    max(4096, n) words each (an even count, so payload element 0 is as aligned as the allocation).  Frames are placed with place();
    address(offset) is the base pointer of a call whose layout has that offset; faults() judges the words after the call.
    On the host (dev=None) the words are a numpy array and address() points into it; with a DeviceHelper the words are uploaded by
    commit() into one torch allocation (256-byte aligned) and faults() downloads them."""

    def __init__(self, n, span, dev=None, band=None):
        self.n = int(n)
        self.band = max(4096, self.n) if band is None else int(band)
        assert self.band >= max(4096, self.n) and self.band % 2 == 0
        self.span = int(span)
        self.words = canary(0, self.band + self.span + self.band)
        self.dev = dev
        self.tensor = None

    def place(self, layout, frames):
        assert layout.span() <= self.span and layout.offset >= 0
        scatter_frames(self.words, self.band, layout, frames)
        return self

    def commit(self):
        """upload the host image (device arenas only); the host copy stays as it was built"""
        self.tensor = self.dev.to_device(self.words)
        assert self.tensor.data_ptr() % 256 == 0
        return self

    def address(self, offset=0):
        assert 0 <= offset <= self.span
        if self.dev is None:
            return self.words.ctypes.data + 8 * (self.band + offset)
        return self.tensor.data_ptr() + 8 * (self.band + offset)

    def view(self, offset, count):
        """host arenas: the payload words offset .. offset + count - 1 as a numpy view (an `out=` argument)"""
        assert self.dev is None and offset >= 0 and offset + count <= self.span
        return self.words[self.band + offset:self.band + offset + count]

    def image(self):
        return self.words if self.dev is None else self.dev.to_host(self.tensor)

    def frames(self, layout, image=None):
        return gather_frames(self.image() if image is None else image, self.band, layout)

    def faults(self, placed, image=None, limit=4):
        return arena_faults(self.image() if image is None else image, self.band, placed, limit)


def arena_for(dev, n, *placed):
    """a committed arena that spans every layout of `placed` ((layout, frames or None), ...), the given frames placed"""
    arena = GuardedArena(n, max(l.span() for l, _ in placed), dev)
    for layout, frames in placed:
        if frames is not None:
            arena.place(layout, frames)
    return arena.commit() if dev is not None else arena


# ---------------------------------------------------------------------------------------
# launches at scale: the oracle per plan, sampled frames, whole-buffer checkers on the device
# ---------------------------------------------------------------------------------------
class OracleRef:
    """the CPU oracle for one plan's moduli and roots"""

    def __init__(self, orc, plan):
        self.orc, self.n = orc, plan.n
        self.q = plan.moduli
        self.psi = [plan.psi(p) for p in range(plan.num_primes)]
        self.tab = [orc.make_tables(q, r, self.n) for q, r in zip(self.q, self.psi)]
        self.itw = [orc.make_inv_tables(q, r, self.n)[0] for q, r in zip(self.q, self.psi)]

    def forward(self, p, x):
        return self.orc.forward(x % np.uint64(self.q[p]), self.q[p], self.tab[p][0], self.tab[p][1], self.n)

    def inverse(self, p, y):
        return self.orc.inverse(y % np.uint64(self.q[p]), self.q[p], self.itw[p], self.n)

    def polymul(self, p, a, b):
        return oracle_polymul(self.orc, a, b, self.q[p], self.psi[p], self.n)


def sample_frames(primes, batch, n, elements=()):
    """global frame indices ([prime][batch] order) to check with the oracle: every prime's boundary frames, and the frames on both
    sides of each of the given element offsets"""
    g = {p * batch + f for p in range(primes) for f in boundary_frames(batch)}
    for e in elements:
        g |= {(e - 1) // n, e // n}
    return sorted(f for f in g if f < primes * batch)


def frames_to_host(t, frames, n):
    """only the listed frames of a device tensor, copied to the host"""
    return {g: t[g * n:(g + 1) * n].cpu().numpy().view(np.uint64) for g in frames}


def thin_frames(frames, keep, limit=16):
    """at most `limit` of the frame numbers `frames`: every one that is in `keep`, the room left filled evenly from the rest"""
    frames = sorted(set(frames))
    kept = [f for f in frames if f in set(keep)]
    rest = [f for f in frames if f not in set(keep)]
    room = min(max(0, limit - len(kept)), len(rest))
    return sorted(kept + [rest[(k * len(rest)) // room] for k in range(room)])


def judged_frames(batch, limit, extra=()):
    """the frames of a large batch to judge with Python integers: the three at either end always, and a thin sample of the boundary frames and of
    `extra`, at most `limit` in all"""
    edges = [0, 1, 2, batch - 3, batch - 2, batch - 1]
    return thin_frames(boundary_frames(batch) + list(extra) + edges, edges, limit=limit)


def resident_grid(torch, n):
    """workgroups of the loop inverse (n = 16384, 32768) that the device holds at once: 4 waves per SIMD of 2^(log n - 5) threads per frame"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * (4 * 256 // (n // 32))


def loop_batch(torch, n):
    """a batch with more frames than resident_grid(torch, n) and a ragged last round"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 2 * cus + 188 if n == 16384 else cus + 144


def companion_batches(plan, main_id, companion_id, limit=1 << 16):
    """(b_lo, b_hi): the largest batch whose forward call the plan's main entry serves and the smallest one its forward companion serves, read back
    through plan.forward_kernel, so that no test states the threshold itself"""
    b_hi = next(b for b in range(1, limit) if plan.forward_kernel(b) == companion_id)
    assert b_hi > 1 and plan.forward_kernel(b_hi - 1) == main_id and plan.forward_kernel(1) == main_id, (b_hi, plan.forward_kernel(b_hi - 1))
    return b_hi - 1, b_hi


def assert_equals_chunked_calls(torch, call, inputs, outputs, batch, chunk):
    """Every word that ONE call on `batch` frames wrote must be the word the same call writes when it is made `chunk` frames at a time (`chunk` small
    enough for one step of any grid).  inputs, outputs: tensors viewed as [slabs][batch][n], the outputs holding what the large call wrote;
    call(ins, outs, frames) makes the call on `frames` frames: ins are dense copies of those frames of the inputs (the call may consume them), outs
    dense buffers filled with -1, both lists in the order given here.  Launches and comparisons run on the current stream, one behind the other."""
    for v in list(inputs) + list(outputs):
        assert v.dim() == 3 and v.shape[1] == batch, tuple(v.shape)
    for f0 in range(0, batch, chunk):
        f1 = min(batch, f0 + chunk)
        ins = [v[:, f0:f1].clone(memory_format=torch.contiguous_format) for v in inputs]
        outs = [torch.full((v.shape[0], f1 - f0, v.shape[2]), -1, dtype=v.dtype, device=v.device) for v in outputs]
        call(ins, outs, f1 - f0)
        for k, (whole, part) in enumerate(zip(outputs, outs)):
            assert torch.equal(whole[:, f0:f1], part), ("output", k, "of the large call differs from the call on frames", f0, f1)


def spread_lazy_(torch, x, moduli, seed):
    """x ([primes][...] on any device, residues in [0, q_p)) += q_p * k in place, k uniform in 0..3 per element: the same residues spread
    over the lazy input range [0, 4q); in chunks, so the temporaries stay small"""
    g = torch.Generator(device=x.device)
    g.manual_seed(seed)
    v = x.view(len(moduli), -1)
    step = 1 << 26
    for p, q in enumerate(moduli):
        for lo in range(0, v.shape[1], step):
            part = v[p, lo:lo + step]
            part += int(q) * torch.randint(0, 4, part.shape, generator=g, device=x.device, dtype=torch.int64)
    return x


def _first_bad(got, want, prime, f0, limit=4):
    """(prime, frame, element) of the first differing words of two [frames][n] chunks, frame numbers from f0"""
    return [(prime, f0 + int(r), int(c)) for r, c in (got != want).nonzero()[:limit].tolist()]


# ---- agx_ntt_automorphism ---------------------------------------------------------------------------------------------------------
def sigma(a, g, n, q):
    """sigma_g of the frames a ([frames][n] or flat, any values: reduced mod q first) under one modulus, from the definition"""
    a = np.asarray(a, dtype=np.uint64).reshape(-1, n) % np.uint64(q)
    e = (np.arange(n, dtype=np.int64) * g) % (2 * n)
    out = np.empty_like(a)
    low = e < n
    out[:, e[low]] = a[:, low]
    out[:, e[~low] - n] = (np.uint64(q) - a[:, ~low]) % np.uint64(q)
    return out.reshape(-1)


def brev(n):
    bits = n.bit_length() - 1
    r = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        r |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    return r


def ntt_pi(n, g):
    """out[p] = in[pi(p)] in NTT form: pi(p) = brev((g brev(p) + (g-1)/2) mod n)"""
    r = brev(n)
    return r[(g * r + (g - 1) // 2) % n]


def check_automorphism_ntt(torch, got, src, batch, n, g, device=None):
    """NTT form on the whole buffer: got.view(-1, n) must equal src.view(-1, n)[:, pi], pi built on the host, compared in chunks of
    frames on `device` (default: where got lives); returns up to 4 (prime, frame, element) of differing words (empty = pass)"""
    device = got.device if device is None else device
    pi = torch.from_numpy(ntt_pi(n, g)).to(device)
    gv, sv = got.view(-1, n), src.view(-1, n)
    step = max(1, (1 << 26) // n)
    bad = []
    for f0 in range(0, gv.shape[0], step):
        want = sv[f0:f0 + step][:, pi]
        if not torch.equal(gv[f0:f0 + step], want):
            bad += [(f // batch, f % batch, e) for _, f, e in _first_bad(gv[f0:f0 + step], want, 0, f0)]
            if len(bad) >= 4:
                break
    return bad[:4]


def check_automorphism_coeff(torch, got, src, moduli, batch, n, g, device=None):
    """coefficient form on the whole buffer, as the gather out[i] = +-src[j mod n], j = g^-1 i mod 2n, minus iff j >= n, with (q - v) % q
    in int64 (q < 2^62; src in [0, 4q) below 2^63 is reduced first); returns up to 4 (prime, frame, element) (empty = pass)"""
    device = got.device if device is None else device
    j = (pow(int(g), -1, 2 * n) * np.arange(n, dtype=np.int64)) % (2 * n)
    idx, neg = torch.from_numpy(j % n).to(device), torch.from_numpy(j >= n).to(device)[None, :]
    gv, sv = got.view(len(moduli), batch, n), src.view(len(moduli), batch, n)
    step = max(1, (1 << 26) // n)
    bad = []
    for p, q in enumerate(moduli):
        for f0 in range(0, batch, step):
            v = sv[p, f0:f0 + step][:, idx] % int(q)
            want = torch.where(neg, (int(q) - v) % int(q), v)
            if not torch.equal(gv[p, f0:f0 + step], want):
                bad += _first_bad(gv[p, f0:f0 + step], want, p, f0)
                if len(bad) >= 4:
                    return bad[:4]
    return bad


# ---- agx_ntt_rescale: the constructed-quotient identity ---------------------------------------------------------------------------
# Slabs 0 .. P-2 of one random [P][batch][n] buffer y are the residues y_i of an integer Y in [0, Q / q_L) (any residues are: CRT), the
# last slab is r in [0, q_L).  X = Y q_L + r < Q has the residues x_i = (y_i (q_L mod q_i) + r mod q_i) mod q_i and x_L = r, so
# floor(X / q_L) = Y, and floor((X + h) / q_L) = Y + [r + h >= q_L] = Y + [r > h], h = (q_L - 1) / 2 (q_L = 2h + 1).
def rescale_identity_constants(moduli):
    """C_i = q_L mod q_i for i < P-1, C_L = 0: the second operand of the product y o C"""
    return [int(moduli[-1]) % int(q) for q in moduli[:-1]] + [0]


def fill_rescale_constants(torch, c, moduli):
    """c ([P][...]): slab i <- C_i"""
    v = c.view(len(moduli), -1)
    for p, k in enumerate(rescale_identity_constants(moduli)):
        v[p].fill_(k)
    return c


def rescale_identity_sum_(torch, x, y, moduli):
    """x ([P][...], holding y o C mod q_i) <- the residues of X in place: x_i = (x_i + r mod q_i) mod q_i (both terms below 2^62: int64
    holds the sum), x_L = r, r the last slab of y"""
    P = len(moduli)
    xv, yv = x.view(P, -1), y.view(P, -1)
    step = 1 << 26
    for lo in range(0, xv.shape[1], step):
        r = yv[P - 1, lo:lo + step]
        for p in range(P - 1):
            part = xv[p, lo:lo + step]
            part += r % int(moduli[p])
            part %= int(moduli[p])
        xv[P - 1, lo:lo + step] = r
    return x


def check_rescale_identity(torch, got, y, moduli, batch, n, mode, device=None):
    """got ([P-1 or more][batch][n], COEFFICIENT form: the call's output taken back by the inverse) on every word: slab i must be y_i
    (mode 0, floor) or (y_i + [r > h]) mod q_i (mode 1, round); returns up to 4 (prime, frame, element) (empty = pass).  `device` is
    accepted like the other checkers'; everything here is computed where the tensors live"""
    P = len(moduli)
    h = (int(moduli[-1]) - 1) // 2
    gv, yv = got.view(-1, batch, n), y.view(P, batch, n)
    step = max(1, (1 << 26) // n)
    bad = []
    for p in range(P - 1):
        for f0 in range(0, batch, step):
            want = yv[p, f0:f0 + step]
            if mode:
                want = (want + (yv[P - 1, f0:f0 + step] > h).to(want.dtype)) % int(moduli[p])
            if not torch.equal(gv[p, f0:f0 + step], want):
                bad += _first_bad(gv[p, f0:f0 + step], want, p, f0)
                if len(bad) >= 4:
                    return bad[:4]
    return bad


def rescale_reference(residues, moduli, mode):
    """Python integers: residues ([P][count] uint64) -> X per coefficient by CRT -> Y = floor((X + {0, h}) / q_L) -> Y mod q_i, [P-1][count]"""
    moduli = [int(q) for q in moduli]
    Q = 1
    for q in moduli:
        Q *= q
    qL = moduli[-1]
    h = (qL - 1) // 2 if mode else 0
    res = np.asarray(residues, dtype=np.uint64).reshape(len(moduli), -1)
    X = np.zeros(res.shape[1], dtype=object)
    for p, q in enumerate(moduli):
        X = X + res[p].astype(object) * ((Q // q) * pow(Q // q, -1, q))
    Y = (X % Q + h) // qL
    return np.stack([(Y % q).astype(np.uint64) for q in moduli[:-1]])


# ---- products by one fixed monomial per prime -------------------------------------------------------------------------------------
def check_fixed_shifts(torch, c, a, moduli, batch, n, shifts, device=None):
    """every frame of prime p of c ([primes][batch][n]) must be X^shifts[p] * a_f mod (X^n + 1, q_p), a in [0, 4q): built with gather /
    where in chunks of frames; returns up to 4 (prime, frame, element) (empty = pass)"""
    device = c.device if device is None else device
    cv, av = c.view(len(moduli), batch, n), a.view(len(moduli), batch, n)
    i = torch.arange(n, dtype=torch.int64, device=device)
    step = max(1, (1 << 26) // n)
    bad = []
    for p, q in enumerate(moduli):
        j = int(shifts[p])
        idx, neg = (i - j) % n, (i < j)[None, :]
        for f0 in range(0, batch, step):
            v = av[p, f0:f0 + step][:, idx] % int(q)
            want = torch.where(neg, (int(q) - v) % int(q), v)
            if not torch.equal(cv[p, f0:f0 + step], want):
                bad += _first_bad(cv[p, f0:f0 + step], want, p, f0)
                if len(bad) >= 4:
                    return bad[:4]
    return bad


# ---------------------------------------------------------------------------------------
# the kernel registry as the tests know it
# ---------------------------------------------------------------------------------------
# registry ids of the product library (what a default or a call-shape selector can reach); every other id is an A/B entry that
# only lib/libagxntt_diag.so carries: tests/test_gpu_diag.py re-runs the id-parametrised tests of test_gpu_parity.py in a child
# process bound to that library
PRODUCT_IDS = ({93, 92, 91, 159, 164, 117, 119, 120, 121, 122, 123} | set(range(150, 159)) | set(range(130, 142))
               | set(range(200, 215)) | set(range(230, 235)) | set(range(240, 245)) | set(range(250, 258)) | set(range(260, 268)))

# every entry of the kernel registry, (id, n, max_bits): the size it serves and the largest modulus its arithmetic admits
# (exact: 62 bits, fast: 61, 16q-lazy: 60)
REGISTRY = [
    (91, 4096, 62), (92, 4096, 61), (93, 4096, 60), (159, 4096, 60), (147, 4096, 60), (161, 4096, 60), (70, 4096, 60),
    # streamed single-frame kernels (lazy, fast, exact): n = 1024 / 2048 / 8192, 16384 (117 + forward companion 164), 32768; A/B twins 115 / 160 / 114
    (150, 1024, 60), (151, 1024, 61), (152, 1024, 62), (153, 2048, 60), (154, 2048, 61), (155, 2048, 62), (156, 8192, 60), (157, 8192, 61), (158, 8192, 62),
    (117, 16384, 60), (164, 16384, 60), (120, 16384, 61), (122, 16384, 62), (115, 16384, 60), (160, 16384, 60),
    (119, 32768, 60), (121, 32768, 61), (123, 32768, 62), (114, 32768, 60),
    # 32-bit arithmetic: tier 2 (every q < 2^30), tier 1 (every q < 2^31)
    (130, 1024, 30), (131, 2048, 30), (132, 4096, 30), (133, 8192, 30), (134, 16384, 30), (135, 32768, 30),
    (136, 1024, 31), (137, 2048, 31), (138, 4096, 31), (139, 8192, 31), (140, 16384, 31), (141, 32768, 31),
    # wave-packed kernels of n = 32 ... 512 (csrc/wp_kernels.hpp): 16q-lazy / fast / exact per size, then the 32-bit tiers
    (200, 32, 60), (201, 32, 61), (202, 32, 62), (203, 64, 60), (204, 64, 61), (205, 64, 62), (206, 128, 60), (207, 128, 61), (208, 128, 62),
    (209, 256, 60), (210, 256, 61), (211, 256, 62), (212, 512, 60), (213, 512, 61), (214, 512, 62),
    (230, 32, 30), (231, 64, 30), (232, 128, 30), (233, 256, 30), (234, 512, 30), (240, 32, 31), (241, 64, 31), (242, 128, 31), (243, 256, 31), (244, 512, 31),
    # n = 2 ... 16: one lane per frame (fast / exact; 32-bit tiers)
    (250, 2, 61), (251, 2, 62), (252, 4, 61), (253, 4, 62), (254, 8, 61), (255, 8, 62), (256, 16, 61), (257, 16, 62),
    (260, 2, 30), (261, 4, 30), (262, 8, 30), (263, 16, 30), (264, 2, 31), (265, 4, 31), (266, 8, 31), (267, 16, 31),
    # A/B shapes of the wave-packed kernels (lib/libagxntt_diag.so)
    (215, 32, 60), (220, 512, 60), (221, 512, 60), (222, 256, 60), (224, 32, 60), (235, 32, 30), (236, 512, 30),
]

# the product entry that admits only moduli 2^60 - c, 0 < c < 2^28 (arithmetic level 3): the forward companion of such plans at n = 4096.  It stands
# apart from REGISTRY, every entry of which the id-parametrised tests select under its widest modulus and under a 30-bit one
Q60C_REGISTRY = [(165, 4096, 60)]

# the product library's registry entries that carry launch_rescale (the A/B twins 70, 114, 115, 147, 160, 161, 221 carry it too; they
# live in the diagnostics library only)
RESCALE_IDS = [91, 92, 93, 150, 151, 152, 153, 154, 155, 156, 157, 158, 117, 120, 122, 119, 121, 123]


def registry_entries(ids):
    """the (id, n, max_bits) entries of REGISTRY for `ids`, in the order of `ids`"""
    by_id = {e[0]: e for e in REGISTRY}
    return [by_id[i] for i in ids]


def select_entry(agx, plan, config):
    """explicit registry entry (AGX_VARIANT_REGBLOCK_BASE + id); A/B ids are skipped unless the diag library is loaded"""
    if config is None or config == "default":
        return
    if config not in PRODUCT_IDS and not agx.LIB_PATH.endswith("libagxntt_diag.so"):
        plan.close()
        pytest.skip(f"registry id {config} lives in lib/libagxntt_diag.so (covered by tests/test_gpu_diag.py)")
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + config)


# ---------------------------------------------------------------------------------------
# launches of more than 2^32 elements (34 GB and more per buffer: an MI355X holds 288 GB)
# ---------------------------------------------------------------------------------------
EDGES = (1 << 28, 1 << 31, 1 << 32)      # 2^31 bytes, 2^31 and 2^32 elements


@pytest.fixture
def big_memory(dev):
    """frees torch's cached blocks before and after, so that the test (and the plans of later tests) can have the memory;
    need(buffers, elements) skips unless 1.1x that much device memory is free"""
    torch = dev.torch
    torch.cuda.empty_cache()

    def need(buffers, elements):
        want = buffers * elements * 8 + (4 << 30)      # + chunked temporaries of the device-side checks
        free, _ = torch.cuda.mem_get_info()
        if free < 1.1 * want:
            pytest.skip(f"needs {1.1 * want / 2**30:.0f} GiB of free device memory, {free / 2**30:.0f} GiB free")

    yield need
    dev.sync()
    torch.cuda.empty_cache()
