"""tools/run_op.py -- launch ONE operation of the engine a fixed number of times (for rocprofv3 --pmc / --kernel-trace
runs on paths bench.py's headline does not cover).
Usage: python3 tools/run_op.py --op {fwd,inv,mul,mulntt,rescale} [--n N --primes P --batch B --bits 60 --oop --launches K --variant ID]
       python3 tools/run_op.py --op auto --form {coeff,ntt} --galois G [--odd --reps 5 ...]   (agx_ntt_automorphism beside a device copy of the same words)
       python3 tools/run_op.py --op extend --src S [--dst T --only {both,fused,pair} --reps 5 ...]   (agx_ntt_basis_extend to NTT form beside the unfused pair)
       python3 tools/run_op.py --op moddown --src S --dst T [--only {all,fused,generic,parent} --reps 7 ...]   (agx_ntt_basis_mod_down: its two routes and the parent's inverse + extend)
Under the profiler: rocprofv3 ... -- python3 tools/run_op.py ...   (the interpreter itself after `--`, never this file: an
`env` shebang hop after the profiler's preload has initialised the GPU is a forbidden exec on this pool)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import agilex_ntt_amd as agx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--op", choices=["fwd", "inv", "mul", "mulntt", "rescale", "auto", "extend", "moddown"], default="inv")
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--primes", type=int, default=4)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--slabs", type=int, default=4)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--bits", type=int, default=60, help="modulus size in bits")
ap.add_argument("--oop", action="store_true", help="forward / inverse out of place (slab i -> slab i+1)")
ap.add_argument("--variant", type=int, default=None, help="registry id (AGX_VARIANT_REGBLOCK_BASE + id)")
ap.add_argument("--ramp-seconds", type=float, default=0.5, help="run the operation this long before the warm-up launches so the GPU clock has ramped, as bench.py does (0 = cold)")
ap.add_argument("--mulsets", type=int, default=0, help="mul: K rotating (a, b) operand sets, c and scratch separate (bench.py's n = 32768 product line); 0 = c aliases a on the slabs")
ap.add_argument("--bcast", action="store_true", help="mulntt: one bhat frame per prime shared by the whole batch (bhat_batch = 1)")
ap.add_argument("--mode", choices=["floor", "round"], default="round", help="rescale: AGX_RESCALE_FLOOR / AGX_RESCALE_ROUND")
ap.add_argument("--inplace", action="store_true", help="rescale: out == x with x's last slab as the scratch (default: out and scratch of their own)")
ap.add_argument("--form", choices=["coeff", "ntt"], default="ntt", help="auto: AGX_FORM_COEFF / AGX_FORM_NTT")
ap.add_argument("--galois", type=int, default=5, help="auto: the Galois element g (odd, below 2n; -1 = 2n - 1, conjugation)")
ap.add_argument("--odd", action="store_true", help="auto: both bases one word past a 16-byte boundary (the NTT form then takes its 8-byte accesses)")
ap.add_argument("--reps", type=int, default=5, help="auto: timed repetitions of --launches calls each, alternating with the copy; medians are reported")
ap.add_argument("--src", type=int, default=2, help="extend: source primes [0, S)")
ap.add_argument("--dst", type=int, default=0, help="extend: target primes [0, T); 0 = every prime of the plan")
ap.add_argument("--only", choices=["both", "fused", "pair", "all", "generic", "parent"], default=None,
                help="extend: time the AGX_FORM_NTT call (fused), the unfused pair, or both alternating (default); moddown: the two-launch route (fused), the "
                     "four-launch route on the same plan (generic: needs lib/libagxntt_diag.so through AGX_NTT_LIB), inverse + extend as before mod_down existed "
                     "(parent), or all alternating (default).  A counter run wants one")
ap.add_argument("--report", type=str, default=None, help="write {calls: ramp + warm-up + timed launches, ms: ...} here (tools/summarize_ops.py)")
args = ap.parse_args()
if args.op == "moddown":
    args.dst = args.dst or 4
    args.primes = args.src + args.dst      # targets [0, T), sources [T, T + S)
args.only = args.only or ("all" if args.op == "moddown" else "both")
plan = agx.Plan(args.n, agx.find_primes(args.bits, args.n, args.primes))
if args.variant is not None:
    plan.set_variant(agx.VARIANT_REGBLOCK_BASE + args.variant)
stream = torch.cuda.current_stream().cuda_stream
per = args.primes * args.batch * args.n


def run_auto():
    """agx_ntt_automorphism and a device-to-device copy of the same [prime][batch][n] words, alternating in one process: both read and
    write 16n bytes per frame, so the copy is the yardstick.  Prints us per call, GB/s and the ratio, each the median of --reps
    repetitions, with the copy's own spread beside it."""
    import statistics
    import time

    g = 2 * args.n - 1 if args.galois < 0 else args.galois
    form = agx.FORM_COEFF if args.form == "coeff" else agx.FORM_NTT
    pad = 2      # words: keeps the shifted views inside their allocations
    src, dst = (torch.empty(per + pad, dtype=torch.int64, device="cuda") for _ in range(2))
    off = 1 if args.odd else 0
    plan.fill_synthetic(src.data_ptr() + 8 * off, args.batch, 0, 42, stream)
    s_view, d_view = src[off:off + per], dst[off:off + per]

    def auto():
        plan.automorphism(s_view.data_ptr(), d_view.data_ptr(), args.batch, g, form, stream)

    def copy():
        d_view.copy_(s_view)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches      # us per call

    t_end = time.perf_counter() + args.ramp_seconds
    while time.perf_counter() < t_end:      # clock ramp, as below
        for _ in range(8):
            auto()
            copy()
        torch.cuda.synchronize()
    t_auto, t_copy = [], []
    for _ in range(args.reps):
        t_auto.append(timed(auto))
        t_copy.append(timed(copy))
    gbs = lambda us: 16.0 * per / us / 1e3      # noqa: E731  (8 bytes read + 8 written per word)
    ma, mc = statistics.median(t_auto), statistics.median(t_copy)
    print(f"auto form={args.form} g={g} n={args.n} primes={args.primes} batch={args.batch} bits={args.bits}{' odd bases' if args.odd else ''}: "
          f"{ma:.1f} us per call, {gbs(ma):.0f} GB/s (min {min(t_auto):.1f} max {max(t_auto):.1f} us); "
          f"copy {mc:.1f} us, {gbs(mc):.0f} GB/s (min {min(t_copy):.1f} max {max(t_copy):.1f} us); ratio auto/copy {ma / mc:.3f}")
    if args.report:
        import json

        json.dump({"us_auto": t_auto, "us_copy": t_copy, "launches": args.launches, "bytes": 16 * per}, open(args.report, "w"))
    plan.close()


def run_extend():
    """agx_ntt_basis_extend from primes [0, S) to [0, T) in AGX_FORM_NTT (one launch where the fused kernel serves) and the unfused pair
    -- the AGX_FORM_COEFF call, then agx_ntt_forward in place on a plan of the target primes -- alternating in one process.  Prints us per
    call (median of --reps repetitions, min and max beside it), the model traffic 8n(S + T) bytes per frame as GB/s, and the ratio."""
    import statistics
    import time

    S, T = args.src, args.dst or args.primes
    basis = plan.basis(0, S, 0, T)
    targets = agx.Plan(args.n, plan.moduli[:T], psi=[plan.psi(p) for p in range(T)])      # the same tables: what the pair's forward runs on
    if args.variant is not None:
        targets.set_variant(agx.VARIANT_REGBLOCK_BASE + args.variant)
    words = args.batch * args.n
    # fill_synthetic writes a slab for EVERY prime of the plan: the buffer holds them all, the call reads the first S (slab i: residues below q_i)
    x = torch.empty(args.primes * words, dtype=torch.int64, device="cuda")
    out = torch.empty(T * words, dtype=torch.int64, device="cuda")
    plan.fill_synthetic(x.data_ptr(), args.batch, 0, 42, stream)

    def fused():
        basis.extend(x.data_ptr(), out.data_ptr(), args.batch, agx.FORM_NTT, stream)

    def pair():
        basis.extend(x.data_ptr(), out.data_ptr(), args.batch, agx.FORM_COEFF, stream)
        targets.forward(out.data_ptr(), out.data_ptr(), args.batch, stream)

    todo = [f for name, f in (("fused", fused), ("pair", pair)) if args.only in ("both", name)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches      # us per call

    t_end = time.perf_counter() + args.ramp_seconds
    while time.perf_counter() < t_end:      # clock ramp, as below
        for _ in range(8):
            for fn in todo:
                fn()
        torch.cuda.synchronize()
    times = {fn.__name__: [] for fn in todo}
    for _ in range(args.reps):
        for fn in todo:
            times[fn.__name__].append(timed(fn))
    model = 8.0 * words * (S + T)      # bytes: every source word read once, every target word written once
    head = f"extend n={args.n} S={S} T={T} batch={args.batch} bits={args.bits} launches_ntt_form={basis.info()[4]}:"
    parts = [f"{name} {statistics.median(t):.1f} us per call (min {min(t):.1f} max {max(t):.1f}), {model / statistics.median(t) / 1e3:.0f} GB/s of model traffic"
             for name, t in times.items()]
    if len(times) == 2:
        parts.append(f"ratio fused/pair {statistics.median(times['fused']) / statistics.median(times['pair']):.3f}")
    print(head, "; ".join(parts))
    if args.report:
        import json

        json.dump({"us": times, "launches": args.launches, "model_bytes": model}, open(args.report, "w"))
    basis.close()
    targets.close()
    plan.close()


def run_moddown():
    """agx_ntt_basis_mod_down from the sources [T, T + S) to the targets [0, T), three ways alternating in one process:
      fused   -- the call as the library routes it (two launches where the fused kernel serves);
      generic -- the same call sent down the four-launch route on the same plan (AGX_NTT_MOD_DOWN_GENERIC=1, honoured by lib/libagxntt_diag.so only);
      parent  -- what the library offered before mod_down: agx_ntt_inverse of the S source slabs on a plan over those primes, then
                 agx_ntt_basis_extend(..., AGX_FORM_NTT); strictly less work (no subtraction from xq, no product by D^-1).
    Prints us per call (median of --reps repetitions of --launches calls, min and max beside it) and the ratios."""
    import statistics
    import time

    S, T = args.src, args.dst
    basis = plan.basis(T, S, 0, T)
    sources = agx.Plan(args.n, plan.moduli[T:], psi=[plan.psi(p) for p in range(T, T + S)])      # the parent's second plan, the same tables
    if args.variant is not None:
        sources.set_variant(agx.VARIANT_REGBLOCK_BASE + args.variant)
    words = args.batch * args.n
    x = torch.empty((T + S) * words, dtype=torch.int64, device="cuda")      # synthetic residues taken as NTT-form words: xq = slabs [0, T), xp = the rest
    out, scratch = torch.empty(T * words, dtype=torch.int64, device="cuda"), torch.empty(S * words, dtype=torch.int64, device="cuda")
    plan.fill_synthetic(x.data_ptr(), args.batch, 0, 42, stream)
    xq, xp = x.data_ptr(), x.data_ptr() + 8 * T * words
    diag = agx.LIB_PATH.endswith("libagxntt_diag.so")
    if args.only in ("all", "generic") and not diag:
        sys.exit("--only generic / all need lib/libagxntt_diag.so: AGX_NTT_LIB=agilex-ntt_amd/lib/libagxntt_diag.so (after `make -C agilex-ntt_amd diag`)")

    def fused():
        basis.mod_down(xq, xp, out.data_ptr(), scratch.data_ptr(), args.batch, stream)

    def generic():
        os.environ["AGX_NTT_MOD_DOWN_GENERIC"] = "1"
        try:
            basis.mod_down(xq, xp, out.data_ptr(), scratch.data_ptr(), args.batch, stream)
        finally:
            os.environ["AGX_NTT_MOD_DOWN_GENERIC"] = "0"

    def parent():
        sources.inverse(xp, scratch.data_ptr(), args.batch, stream)
        basis.extend(scratch.data_ptr(), out.data_ptr(), args.batch, agx.FORM_NTT, stream)

    launches = {"fused": basis.mod_down_launches(), "parent": 1 + basis.info()[4]}
    if diag:
        os.environ["AGX_NTT_MOD_DOWN_GENERIC"] = "1"
        launches["generic"] = basis.mod_down_launches()
        os.environ["AGX_NTT_MOD_DOWN_GENERIC"] = "0"
    todo = [f for f in (fused, generic, parent) if args.only in ("all", f.__name__)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches      # us per call

    t_end = time.perf_counter() + args.ramp_seconds
    while time.perf_counter() < t_end:      # clock ramp
        for _ in range(8):
            for fn in todo:
                fn()
        torch.cuda.synchronize()
    times = {fn.__name__: [] for fn in todo}
    for _ in range(args.reps):
        for fn in todo:
            times[fn.__name__].append(timed(fn))
    med = {k: statistics.median(t) for k, t in times.items()}
    head = f"moddown n={args.n} S={S} T={T} batch={args.batch} bits={args.bits}:"
    parts = [f"{name} ({launches[name]} launches) {med[name]:.1f} us per call (min {min(t):.1f} max {max(t):.1f})" for name, t in times.items()]
    parts += [f"ratio fused/{other} {med['fused'] / med[other]:.3f}" for other in ("generic", "parent") if "fused" in med and other in med]
    print(head, "; ".join(parts))
    if args.report:
        import json

        json.dump({"us": times, "launches": args.launches, "kernel_launches": launches}, open(args.report, "w"))
    basis.close()
    sources.close()
    plan.close()


if args.op == "auto":
    run_auto()
    sys.exit(0)
if args.op == "moddown":
    run_moddown()
    sys.exit(0)
if args.op == "extend":
    run_extend()
    sys.exit(0)
slabs = [torch.empty(per, dtype=torch.int64, device="cuda") for _ in range(args.slabs)]
for i, s in enumerate(slabs):
    plan.fill_synthetic(s.data_ptr(), args.batch, i * args.batch, 42, stream)
scratch = torch.empty(per, dtype=torch.int64, device="cuda")
sets, cbuf = [], None
if args.op in ("mul", "mulntt") and args.mulsets:
    sets = [[torch.empty(per, dtype=torch.int64, device="cuda") for _ in range(2)] for _ in range(args.mulsets)]
    for k, (a, b) in enumerate(sets):
        plan.fill_synthetic(a.data_ptr(), args.batch, 2 * k * args.batch, 42, stream)
        plan.fill_synthetic(b.data_ptr(), args.batch, (2 * k + 1) * args.batch, 42, stream)
    cbuf = torch.empty(per, dtype=torch.int64, device="cuda")
# mulntt: the second operand of every pair is transformed once, outside the timed region (agx_ntt_polymul_ntt's bhat); --bcast keeps
# one frame per prime of it
hats = {}
if args.op == "mulntt":
    for b in ([s[1] for s in sets] if sets else slabs):
        if args.bcast:
            b1 = b.view(args.primes, args.batch, args.n)[:, 0].contiguous().view(-1)
            h = torch.empty_like(b1)
            plan.forward(b1.data_ptr(), h.data_ptr(), 1, stream)
        else:
            h = torch.empty_like(b)
            plan.forward(b.data_ptr(), h.data_ptr(), args.batch, stream)
        hats[b.data_ptr()] = h
    torch.cuda.synchronize()
bhat_batch = 1 if args.bcast else args.batch
# rescale: x = a slab ([P][batch][n], the synthetic residues taken as NTT-form words), out [P-1][batch][n] and batch*n words of scratch
rs_mode = agx.RESCALE_FLOOR if args.mode == "floor" else agx.RESCALE_ROUND
rs_out = torch.empty((args.primes - 1) * args.batch * args.n, dtype=torch.int64, device="cuda") if args.op == "rescale" else None


def run(i):
    if sets:
        a, b = sets[i % len(sets)]
        if args.op == "mulntt":
            plan.polymul_ntt(a.data_ptr(), hats[b.data_ptr()].data_ptr(), cbuf.data_ptr(), args.batch, bhat_batch, stream)
            return
        plan.polymul(a.data_ptr(), b.data_ptr(), cbuf.data_ptr(), scratch.data_ptr(), args.batch, stream)
        return
    a, b = slabs[i % args.slabs], slabs[(i + 1) % args.slabs]
    if args.op == "rescale":
        if args.inplace:
            plan.rescale(a.data_ptr(), a.data_ptr(), a.data_ptr() + 8 * (args.primes - 1) * args.batch * args.n, args.batch, rs_mode, stream)
        else:
            plan.rescale(a.data_ptr(), rs_out.data_ptr(), scratch.data_ptr(), args.batch, rs_mode, stream)
        return
    dst = b if args.oop else a
    if args.op == "fwd":
        plan.forward(a.data_ptr(), dst.data_ptr(), args.batch, stream)
    elif args.op == "inv":
        plan.inverse(a.data_ptr(), dst.data_ptr(), args.batch, stream)
    elif args.op == "mul":
        plan.polymul(a.data_ptr(), b.data_ptr(), a.data_ptr(), scratch.data_ptr(), args.batch, stream)
    else:
        plan.polymul_ntt(a.data_ptr(), hats[b.data_ptr()].data_ptr(), a.data_ptr(), args.batch, bhat_batch, stream)


import time  # noqa: E402

calls = 0
t_end = time.perf_counter() + args.ramp_seconds
while time.perf_counter() < t_end:      # clock ramp (bench.py: the first ~100 ms of work after an idle period run ~10 % slower)
    for i in range(16):
        run(calls)
        calls += 1
    torch.cuda.synchronize()
for i in range(5):
    run(i)
calls += 5
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for i in range(args.launches):
    run(i)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / args.launches
calls += args.launches
if args.report:
    import json

    json.dump({"calls": calls, "timed": args.launches, "ms_per_launch": ms}, open(args.report, "w"))
if args.op == "rescale":
    print(f"rescale ({args.mode}{', in place' if args.inplace else ''}) n={args.n} primes={args.primes} batch={args.batch} bits={args.bits}: {ms * 1e3:.1f} us per call, "
          f"{args.batch / ms / 1e3:.3f} M RNS frames/s")
else:
    print(f"{args.op} n={args.n} primes={args.primes} batch={args.batch}: {ms:.4f} ms per launch, {args.primes * args.batch / ms / 1e3:.2f} M units/s")
plan.close()
