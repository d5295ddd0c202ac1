"""tools/run_op.py -- launch ONE operation of the engine a fixed number of times (for rocprofv3 --pmc / --kernel-trace
runs on paths bench.py's headline does not cover).
Usage: python3 tools/run_op.py --op {fwd,inv,mul,mulntt,rescale} [--n N --primes P --batch B --bits 60 --oop --launches K --variant ID]
       python3 tools/run_op.py --op auto --form {coeff,ntt} --galois G [--odd --reps 5 ...]   (agx_ntt_automorphism beside a device copy of the same words)
       python3 tools/run_op.py --op extend --src S [--dst T --only {both,fused,pair} --reps 5 ...]   (agx_ntt_basis_extend to NTT form beside the unfused pair)
       python3 tools/run_op.py --op moddown --src S --dst T [--only {all,fused,generic,parent,modes} --mode {floor,round} --plain T --reps 7 ...]   (agx_ntt_basis_mod_down: its two routes and the parent's inverse + extend)
       python3 tools/run_op.py --op bfvconv --src S --dst T [--only {all,exact,mont,parent,copy} --reps 7 ...]   (agx_ntt_basis_extend_exact / _mont, coefficient form, beside agx_ntt_basis_extend into T + 1 targets and a copy of the model's bytes)
       python3 tools/run_op.py --op quotient --qcount L --src K [--only {all,quotient,composition,copy} --reps 7 ...]   (agx_ntt_basis_quotient beside the six-call composition it replaces and a copy of its model bytes)
       python3 tools/run_op.py --op plain --qcount L [--reps 7 ...]   (agx_ntt_plain_scale_down, _scale_up and _lift in both forms beside a copy of each call's model bytes and the plan's inverse / forward alone)
       python3 tools/run_op.py --op ckks --qcount L [--reps 7 ...]   (agx_ntt_ckks_encode and _decode with full slots in both forms beside a copy of the call's model bytes and the plan's forward / inverse alone)
       python3 tools/run_op.py --op batch --qcount L [--reps 7 ...]   (agx_ntt_batch_encode and _decode at t = 65537 beside the inner plan's inverse / forward alone and a copy of the permutation's 16 n bytes per frame;
                                                                    agx_ntt_plain_reduce beside agx_ntt_plain_scale_down on the same L slabs)
       python3 tools/run_op.py --op sample --kind {uniform,ternary,cbd} [--primes L --eta 21 --reps 7 ...]   (agx_ntt_sample_*: a draw, in both forms for the small kinds, beside a device fill of the same bytes and the plan's forward;
                                                                   uniform also under the primes just above 2^60, where every cell takes two blocks or more)
       python3 tools/run_op.py --op inner --terms T [--outputs 2 --bcast --only {all,inner,copy,parent} --reps 7 ...]   (agx_ntt_inner_product beside a copy of its model traffic and pointwise-and-add)
       python3 tools/run_op.py --op ring --kind {add,sub,negate,add_galois,tensor} [--primes 6 --first 0 --count 4 --galois G --only {all,ring,copy,parent} --reps 7 ...]   (a ring call beside a copy of its model bytes and what it replaces)
       python3 tools/run_op.py --op keyswitch --qcount Q [--pfirst F --pcount K --alpha A --reps 7 ...]   (agx_ntt_keyswitch_apply beside the composition of public calls, and the stages)
       python3 tools/run_op.py --op hoist --qcount Q --rotations R [R ...] [--galois G --pfirst F --pcount K --alpha A --reps 7 ...]   (hoisted rotations: agx_ntt_inner_product_galois
                                                                   beside the plain kernel and automorphism + inner product; decompose + R apply_decomposed beside R automorphism + apply)
       python3 tools/run_op.py --op dhoist --qcount Q --rotations R [R ...] [--galois G --pfirst F --pcount K --alpha A --reps 7 ...]   (double-hoisted linear transforms:
                                                                   agx_ntt_keyswitch_accumulate_decomposed beside the gathered inner product and a copy of its model bytes; an R-term
                                                                   transform with ONE ModDown pair beside apply_decomposed per rotation)
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
ap.add_argument("--op", choices=["fwd", "inv", "mul", "mulntt", "rescale", "auto", "extend", "moddown", "bfvconv", "inner", "keyswitch", "hoist", "dhoist", "ring", "quotient", "plain", "sample", "ckks", "batch"], default="inv")
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
ap.add_argument("--mode", choices=["floor", "round"], default=None,
                help="rescale (default round), moddown (default floor: agx_ntt_basis_mod_down_mode's mode): AGX_RESCALE_FLOOR / AGX_RESCALE_ROUND")
ap.add_argument("--plain", type=int, default=1, metavar="T", help="moddown: the basis' plaintext modulus t (agx_ntt_basis_create_plain); 1 = the ordinary basis")
ap.add_argument("--inplace", action="store_true", help="rescale: out == x with x's last slab as the scratch (default: out and scratch of their own)")
ap.add_argument("--form", choices=["coeff", "ntt"], default="ntt", help="auto: AGX_FORM_COEFF / AGX_FORM_NTT")
ap.add_argument("--galois", type=int, default=5, help="auto: the Galois element g (odd, below 2n; -1 = 2n - 1, conjugation)")
ap.add_argument("--odd", action="store_true", help="auto: both bases one word past a 16-byte boundary (the NTT form then takes its 8-byte accesses)")
ap.add_argument("--reps", type=int, default=5, help="auto: timed repetitions of --launches calls each, alternating with the copy; medians are reported")
ap.add_argument("--src", type=int, default=2, help="extend: source primes [0, S)")
ap.add_argument("--dst", type=int, default=0, help="extend: target primes [0, T); 0 = every prime of the plan")
ap.add_argument("--only", choices=["both", "fused", "pair", "all", "generic", "parent", "modes", "inner", "copy", "ring", "exact", "mont", "quotient", "composition"], default=None,
                help="extend: time the AGX_FORM_NTT call (fused), the unfused pair, or both alternating (default); moddown: the two-launch route (fused), the "
                     "four-launch route on the same plan (generic: needs lib/libagxntt_diag.so through AGX_NTT_LIB), inverse + extend as before mod_down existed "
                     "(parent), or all alternating (default).  A counter run wants one")
ap.add_argument("--terms", type=int, default=2, help="inner: terms of the sum (1 .. 16)")
ap.add_argument("--outputs", type=int, default=2, help="inner: outputs (1 or 2)")
ap.add_argument("--kind", choices=["add", "sub", "negate", "add_galois", "tensor", "uniform", "ternary", "cbd"], default=None,
                help="ring: the call to time (default add); sample: the draw to time (default uniform)")
ap.add_argument("--eta", type=int, default=21, help="sample --kind cbd: the width eta (1 .. 32)")
ap.add_argument("--first", type=int, default=0, help="ring: the first plan prime of the range")
ap.add_argument("--count", type=int, default=4, help="ring: primes in the range")
ap.add_argument("--qcount", type=int, default=4, help="keyswitch: Q = primes [0, qcount)")
ap.add_argument("--pfirst", type=int, default=None, help="keyswitch: the special primes start here (default: qcount, the top level)")
ap.add_argument("--pcount", type=int, default=2, help="keyswitch: special primes")
ap.add_argument("--alpha", type=int, default=2, help="keyswitch: primes per digit")
ap.add_argument("--rotations", type=int, nargs="+", default=[8], help="hoist, dhoist: rotation counts R to time; rotation r uses the element galois^(r + 1) mod 2n")
ap.add_argument("--report", type=str, default=None, help="write {calls: ramp + warm-up + timed launches, ms: ...} here (tools/summarize_ops.py)")
args = ap.parse_args()
args.mode = args.mode or ("floor" if args.op == "moddown" else "round")
args.kind = args.kind or ("uniform" if args.op == "sample" else "add")
if args.op == "moddown":
    args.dst = args.dst or 4
    args.primes = args.src + args.dst      # targets [0, T), sources [T, T + S)
if args.op == "bfvconv":
    args.dst = args.dst or 3
    args.primes = args.src + args.dst + 1      # sources [0, S), targets [S, S + T), the auxiliary prime S + T
if args.op in ("keyswitch", "hoist", "dhoist"):
    args.pfirst = args.qcount if args.pfirst is None else args.pfirst
    args.primes = args.pfirst + args.pcount
if args.op == "quotient":
    args.primes = args.qcount + args.src + 1      # Q = [0, L), B = [L, L + K), the auxiliary prime L + K
if args.op == "plain":
    args.primes = args.qcount + 1      # Q = [0, L), gamma = L
if args.op == "ckks":
    args.primes = args.qcount      # the handle's primes [0, L), every one in use
if args.op == "batch":
    args.primes = args.qcount + 1      # Q = [0, L), gamma = L, for the plaintext handle; the batching handle has a plan of its own
args.only = args.only or ("all" if args.op in ("moddown", "bfvconv", "quotient") else "both")
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
    The call is agx_ntt_basis_mod_down_mode in --mode (default floor) on a basis with the plaintext modulus --plain (default 1: the ordinary basis).
    --only modes times that call four ways instead, alternating: floor and round on the ordinary basis, plain_floor and plain_round on a basis with
    t = --plain (65537 when --plain is 1).
    Prints us per call (median of --reps repetitions of --launches calls, min and max beside it) and the ratios."""
    import statistics
    import time

    S, T = args.src, args.dst
    mode = agx.RESCALE_ROUND if args.mode == "round" else agx.RESCALE_FLOOR
    basis = plan.basis(T, S, 0, T, t=args.plain)
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
        basis.mod_down(xq, xp, out.data_ptr(), scratch.data_ptr(), args.batch, stream, mode)

    def generic():
        os.environ["AGX_NTT_MOD_DOWN_GENERIC"] = "1"
        try:
            basis.mod_down(xq, xp, out.data_ptr(), scratch.data_ptr(), args.batch, stream, mode)
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
    plain = None
    if args.only == "modes":
        plain = plan.basis(T, S, 0, T, t=65537 if args.plain == 1 else args.plain)
        ordinary = plan.basis(T, S, 0, T)

        def form(name, b, m):
            def call():
                b.mod_down(xq, xp, out.data_ptr(), scratch.data_ptr(), args.batch, stream, m)
            call.__name__ = name
            launches[name] = b.mod_down_launches()
            return call

        todo = [form("floor", ordinary, agx.RESCALE_FLOOR), form("round", ordinary, agx.RESCALE_ROUND), form("plain_floor", plain, agx.RESCALE_FLOOR),
                form("plain_round", plain, agx.RESCALE_ROUND)]

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
    head = f"moddown n={args.n} S={S} T={T} batch={args.batch} bits={args.bits} mode={args.mode} t={args.plain}:"
    parts = [f"{name} ({launches[name]} launches) {med[name]:.1f} us per call (min {min(t):.1f} max {max(t):.1f})" for name, t in times.items()]
    parts += [f"ratio fused/{other} {med['fused'] / med[other]:.3f}" for other in ("generic", "parent") if "fused" in med and other in med]
    parts += [f"ratio {name}/floor {med[name] / med['floor']:.3f}" for name in ("round", "plain_floor", "plain_round") if "floor" in med and name in med]
    print(head, "; ".join(parts))
    if args.report:
        import json

        json.dump({"us": times, "launches": args.launches, "kernel_launches": launches}, open(args.report, "w"))
    basis.close()
    if plain is not None:
        plain.close()
        ordinary.close()
    sources.close()
    plan.close()


def _alternate(todo):
    """0.5 s of the forms first (clock ramp), then --reps repetitions of groups of --launches calls, the forms alternating group by group, device
    events around every group: {name: [us per call]}"""
    import time

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.launches

    t_end = time.perf_counter() + args.ramp_seconds
    while True:
        for fn in todo:
            for _ in range(4):
                fn()
        torch.cuda.synchronize()
        if time.perf_counter() >= t_end:
            break
    times = {fn.__name__: [] for fn in todo}
    for _ in range(args.reps):
        for fn in todo:
            times[fn.__name__].append(timed(fn))
    return times


def _fmt(t):
    import statistics

    return f"{statistics.median(t):.1f} ({min(t):.1f} ... {max(t):.1f})"


def run_quotient():
    """agx_ntt_basis_quotient with Q = [0, L), B = [L, L + K) and m = L + K (--qcount L, --src K), the scratch the operand as in the INTEGRATION.md listing,
    alternating in one process with the six-call composition it replaces -- agx_ntt_mul_add_galois by a frame of t's, agx_ntt_basis_mod_down (sources Q,
    targets Bsk, the Q slabs given up), agx_ntt_inverse on Bsk through a second plan, agx_ntt_basis_extend_exact to NTT form -- and with a device copy of
    the call's model bytes, 8 (2L + K + 1) per coefficient (L + K + 1 slabs read, L written).  Both forms overwrite their operand; any words are NTT-form
    words, so the groups run on what the last call left.  Prints us per call: median (min ... max) of --reps groups of --launches calls."""
    import statistics

    L, K, t = args.qcount, args.src, 65537
    W, words = L + K + 1, args.batch * args.n
    basis = plan.basis_quotient(L, K, 0, L, L + K, t)
    fast_floor, to_q = plan.basis(0, L, L, K + 1), plan.basis_aux(L, K, 0, L, L + K)
    plan_bsk = agx.Plan(args.n, plan.moduli[L:], psi=[plan.psi(k) for k in range(L, W)])
    x = torch.empty(W * words, dtype=torch.int64, device="cuda")
    out = torch.empty(L * words, dtype=torch.int64, device="cuda")
    floor_hat, floor_coeff = (torch.empty((K + 1) * words, dtype=torch.int64, device="cuda") for _ in range(2))
    t_hat = torch.full((W * args.n,), t, dtype=torch.int64, device="cuda")
    plan.fill_synthetic(x.data_ptr(), args.batch, 0, 42, stream)
    half = (2 * L + K + 1) * words // 2      # a copy reads and writes this many words: together the model's bytes
    c_src, c_dst = (torch.empty(half, dtype=torch.int64, device="cuda") for _ in range(2))
    p = x.data_ptr()

    def quotient():
        basis.quotient(p, out.data_ptr(), p, args.batch, stream)

    def composition():
        plan.mul_add_galois(t_hat.data_ptr(), p, p, args.batch, 1, 1, False, 0, W, stream)
        fast_floor.mod_down(p + 8 * L * words, p, floor_hat.data_ptr(), p, args.batch, stream)
        plan_bsk.inverse(floor_hat.data_ptr(), floor_coeff.data_ptr(), args.batch, stream)
        to_q.extend_exact(floor_coeff.data_ptr(), floor_coeff.data_ptr() + 8 * K * words, out.data_ptr(), args.batch, agx.FORM_NTT, stream)

    def copy():
        c_dst.copy_(c_src)

    todo = [f for name, f in (("quotient", quotient), ("composition", composition), ("copy", copy)) if args.only in ("all", name)]
    times = _alternate(todo)
    launches = {"quotient": basis.quotient_info()[2], "composition": 1 + fast_floor.mod_down_launches() + 1 + to_q.aux_info()[2]}
    print(f"quotient n={args.n} L={L} K={K} batch={args.batch} bits={args.bits} launches {launches}:", "; ".join(f"{name} {_fmt(v)} us" for name, v in times.items()))
    med = {k: statistics.median(v) for k, v in times.items()}
    if "quotient" in med:
        print("  " + "  ".join(f"quotient/{name} {med['quotient'] / med[name]:.3f}" for name in ("composition", "copy") if name in med))
    if args.report:
        import json

        json.dump({"us": times, "launches": args.launches, "kernel_launches": launches, "model_bytes": 16.0 * half}, open(args.report, "w"))
    for h in (basis, fast_floor, to_q, plan_bsk):
        h.close()
    plan.close()


def run_plain():
    """agx_ntt_plain_scale_down (the scratch the operand), _scale_up and _lift in both forms with Q = [0, L) and gamma = plan prime L (--qcount L), t = 65537,
    alternating in one process with the plan's inverse and forward alone on the same Q slabs (agx_ntt_inverse_range / agx_ntt_forward_range, in place) and
    with a device copy of each call's model bytes: 8 (L + 1) per coefficient for the three streaming kernels (scale_down's, scale_up's and lift's coefficient
    form).  scale_down overwrites its operand; any words are NTT-form words, so the groups run on what the last call left.  Prints us per call: median
    (min ... max) of --reps groups of --launches calls; scale_down less the inverse alone and the NTT forms less the forward alone estimate the streaming
    kernels where they cannot be timed apart."""
    import statistics

    L, t = args.qcount, 65537
    words = args.batch * args.n
    plain = plan.plain(0, L, L, t)
    x = torch.empty(plan.num_primes * words, dtype=torch.int64, device="cuda")      # agx_ntt_fill_synthetic writes every slab of the plan, gamma's too; slabs [0, L) are read
    out = torch.empty(L * words, dtype=torch.int64, device="cuda")
    m, msg = (torch.empty(words, dtype=torch.int64, device="cuda") for _ in range(2))
    plan.fill_synthetic(x.data_ptr(), args.batch, 0, 42, stream)
    m.copy_(x[:words])      # any 64-bit words are plaintext words
    half = (L + 1) * words // 2      # a copy reads and writes this many words: together the model's bytes of one streaming kernel
    c_src, c_dst = (torch.empty(half, dtype=torch.int64, device="cuda") for _ in range(2))
    p = x.data_ptr()

    def scale_down():
        plain.scale_down(p, msg.data_ptr(), p, args.batch, stream)

    def inverse():
        plan.inverse_range(p, p, args.batch, 0, L, stream)

    def scale_up_coeff():
        plain.scale_up(m.data_ptr(), out.data_ptr(), args.batch, agx.FORM_COEFF, stream)

    def lift_coeff():
        plain.lift(m.data_ptr(), out.data_ptr(), args.batch, agx.FORM_COEFF, stream)

    def scale_up_ntt():
        plain.scale_up(m.data_ptr(), out.data_ptr(), args.batch, agx.FORM_NTT, stream)

    def lift_ntt():
        plain.lift(m.data_ptr(), out.data_ptr(), args.batch, agx.FORM_NTT, stream)

    def forward():
        plan.forward_range(out.data_ptr(), out.data_ptr(), args.batch, 0, L, stream)

    def copy():
        c_dst.copy_(c_src)

    times = _alternate([scale_down, inverse, scale_up_coeff, lift_coeff, scale_up_ntt, lift_ntt, forward, copy])
    info = plain.info()
    print(f"plain n={args.n} L={L} batch={args.batch} bits={args.bits} t={t} launches scale_down {info[4]} ntt form {info[5]}:")
    for name, v in times.items():
        print(f"  {name} {_fmt(v)} us")
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"  scale_down - inverse {med['scale_down'] - med['inverse']:.1f} us = {(med['scale_down'] - med['inverse']) / med['copy']:.3f} of the copy;  "
          f"scale_up_coeff/copy {med['scale_up_coeff'] / med['copy']:.3f}  lift_coeff/copy {med['lift_coeff'] / med['copy']:.3f};  "
          f"scale_down/inverse {med['scale_down'] / med['inverse']:.3f}  scale_up_ntt/(forward + copy) {med['scale_up_ntt'] / (med['forward'] + med['copy']):.3f}")
    if args.report:
        import json

        json.dump({"us": times, "launches": args.launches, "kernel_launches": {"scale_down": info[4], "ntt_form": info[5]}, "model_bytes": 16.0 * half}, open(args.report, "w"))
    plain.close()
    plan.close()


def run_ckks():
    """agx_ntt_ckks_encode and agx_ntt_ckks_decode with full slots (s = n / 2), scale 2^40 and l = --qcount primes, in both forms, alternating in one process
    with the plan's forward and inverse alone on the same slabs (agx_ntt_forward_range / agx_ntt_inverse_range, in place) and with a device copy of a call's
    model bytes, 16 s + 8 n l per frame.  The slots are uniform in the unit square; decode reads what encode wrote (NTT-form decode gives up its operand, so
    its groups run on what the last call left: any words serve).  Prints us per call: median (min ... max) of --reps groups of --launches calls."""
    import statistics

    L, n, batch, s, scale = args.qcount, args.n, args.batch, args.n // 2, 2.0 ** 40
    ck = plan.ckks(0, L)
    words = batch * n
    z = torch.rand(2 * batch * s, dtype=torch.float64, device="cuda") * 2 - 1
    back = torch.empty_like(z)
    out = torch.empty(L * words, dtype=torch.int64, device="cuda")
    hat = torch.empty(L * words, dtype=torch.int64, device="cuda")
    half = (2 * batch * s + L * words) // 2      # a copy reads and writes this many words: together the model's bytes of one call
    c_src, c_dst = (torch.empty(half, dtype=torch.int64, device="cuda") for _ in range(2))
    ck.encode(z.data_ptr(), s, scale, hat.data_ptr(), batch, L, agx.FORM_NTT, stream)

    def encode_coeff():
        ck.encode(z.data_ptr(), s, scale, out.data_ptr(), batch, L, agx.FORM_COEFF, stream)

    def encode_ntt():
        ck.encode(z.data_ptr(), s, scale, hat.data_ptr(), batch, L, agx.FORM_NTT, stream)

    def decode_coeff():
        ck.decode(out.data_ptr(), agx.FORM_COEFF, L, scale, back.data_ptr(), s, None, batch, stream)

    def decode_ntt():
        ck.decode(hat.data_ptr(), agx.FORM_NTT, L, scale, back.data_ptr(), s, hat.data_ptr(), batch, stream)

    def forward():
        plan.forward_range(hat.data_ptr(), hat.data_ptr(), batch, 0, L, stream)

    def inverse():
        plan.inverse_range(hat.data_ptr(), hat.data_ptr(), batch, 0, L, stream)

    def copy():
        c_dst.copy_(c_src)

    times = _alternate([encode_coeff, decode_coeff, encode_ntt, decode_ntt, forward, inverse, copy])
    info = ck.info()
    print(f"ckks n={n} l={L} batch={batch} bits={args.bits} slots={s} launches encode ntt {info[3]} decode ntt {info[4]}; model bytes per call {16 * half}:")
    for name, v in times.items():
        print(f"  {name} {_fmt(v)} us")
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"  encode_coeff/copy {med['encode_coeff'] / med['copy']:.3f}  decode_coeff/copy {med['decode_coeff'] / med['copy']:.3f};  "
          f"encode_ntt/(forward + copy) {med['encode_ntt'] / (med['forward'] + med['copy']):.3f}  decode_ntt/(inverse + copy) {med['decode_ntt'] / (med['inverse'] + med['copy']):.3f}")
    if args.report:
        import json

        json.dump({"us": times, "launches": args.launches, "kernel_launches": {"encode_ntt": info[3], "decode_ntt": info[4]}, "model_bytes": 16.0 * half}, open(args.report, "w"))
    ck.close()
    plan.close()


def run_batch():
    """agx_ntt_batch_encode and agx_ntt_batch_decode (the scratch the operand) at t = 65537, alternating in one process with the inner plan's inverse and
    forward alone on the same frames (agx_ntt_inverse / agx_ntt_forward on the plan agx_ntt_batch_plan lends, in place) and with a device copy of the
    permutation's bytes, 16 n per frame; then agx_ntt_plain_reduce beside agx_ntt_plain_scale_down on the same L = --qcount slabs (the scratch the operand:
    any words serve as the next call's input) and a copy of their kernel's 8 (L + 1) bytes per coefficient.  The permutation kernel has no call of its own:
    its time is encode less the inverse, or decode less the forward, a difference of two medians.  The other gather side (scattered writes) is a library of
    its own, built with EXTRA=-DAGX_BATCH_SCATTER and loaded through AGX_NTT_LIB: run this op once per library, alternating.  Prints us per call: median
    (min ... max)."""
    import statistics

    L, n, batch, t = args.qcount, args.n, args.batch, 65537
    words = batch * n
    bt = agx.Batch(n, t)
    inner = bt.plan()
    z = torch.randint(0, 1 << 62, (words,), dtype=torch.int64, device="cuda")
    m, back = torch.empty_like(z), torch.empty_like(z)
    c_src, c_dst = torch.empty_like(z), torch.empty_like(z)      # a copy reads and writes 8 bytes per word: the permutation's 16 n per frame
    pt = plan.plain(0, L, L, t)
    x = torch.empty(L * words, dtype=torch.int64, device="cuda")
    plan.sample_uniform(bytes(range(32)), 0, x.data_ptr(), batch, 0, 0, L, stream)
    half = (L + 1) * words // 2
    r_src, r_dst = (torch.empty(half, dtype=torch.int64, device="cuda") for _ in range(2))
    bt.encode(z.data_ptr(), m.data_ptr(), batch, stream)

    def encode():
        bt.encode(z.data_ptr(), m.data_ptr(), batch, stream)

    def decode():
        bt.decode(m.data_ptr(), back.data_ptr(), m.data_ptr(), batch, stream)

    def inner_inverse():
        agx._check(agx.lib().agx_ntt_inverse(inner, m.data_ptr(), m.data_ptr(), batch, stream), "inverse")

    def inner_forward():
        agx._check(agx.lib().agx_ntt_forward(inner, m.data_ptr(), m.data_ptr(), batch, stream), "forward")

    def copy():
        c_dst.copy_(c_src)

    def reduce():
        pt.reduce(x.data_ptr(), back.data_ptr(), x.data_ptr(), batch, 3, stream)

    def scale_down():
        pt.scale_down(x.data_ptr(), back.data_ptr(), x.data_ptr(), batch, stream)

    def inverse():
        plan.inverse_range(x.data_ptr(), x.data_ptr(), batch, 0, L, stream)

    def copy_rows():
        r_dst.copy_(r_src)

    times = _alternate([encode, decode, inner_inverse, inner_forward, copy, reduce, scale_down, inverse, copy_rows])
    info = bt.info()
    print(f"batch n={n} t={t} batch={batch} launches encode {info[3]} decode {info[4]}; plain_reduce l={L} bits={args.bits}:")
    for name, v in times.items():
        print(f"  {name} {_fmt(v)} us")
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"  (encode - inner_inverse)/copy {(med['encode'] - med['inner_inverse']) / med['copy']:.3f}  (decode - inner_forward)/copy {(med['decode'] - med['inner_forward']) / med['copy']:.3f};  "
          f"encode/(inner_inverse + copy) {med['encode'] / (med['inner_inverse'] + med['copy']):.3f}  decode/(inner_forward + copy) {med['decode'] / (med['inner_forward'] + med['copy']):.3f};  "
          f"reduce/scale_down {med['reduce'] / med['scale_down']:.3f}  (reduce - inverse)/copy_rows {(med['reduce'] - med['inverse']) / med['copy_rows']:.3f}")
    if args.report:
        import json

        json.dump({"us": times, "launches": args.launches, "kernel_launches": {"encode": info[3], "decode": info[4]}}, open(args.report, "w"))
    pt.close()
    bt.close()
    plan.close()


def _primes_above(bound, n, count):
    """the `count` smallest primes = 1 (mod 2n) above `bound` < 2^62 (Miller-Rabin on the bases that decide every 64-bit number)"""
    def is_prime(m):
        if m < 2 or any(m % p == 0 and m != p for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)):
            return False
        d, r = m - 1, 0
        while d % 2 == 0:
            d, r = d // 2, r + 1
        for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
            x = pow(a, d, m)
            if a % m == 0 or x in (1, m - 1):
                continue
            for _ in range(r - 1):
                x = x * x % m
                if x == m - 1:
                    break
            else:
                return False
        return True

    out, c = [], bound // (2 * n) * (2 * n) + 1
    while len(out) < count:
        if c > bound and is_prime(c):
            out.append(c)
        c += 2 * n
    return out


def run_sample():
    """agx_ntt_sample_uniform / _ternary / _cbd (--kind) on the plan's --primes L primes (60-bit: q = 2^60 - c, one block per cell), alternating in one
    process with (a) a device fill that writes the same 8 L bytes per coefficient and (b) the plan's forward on the same slabs, in place.  The small kinds are
    timed in both forms; uniform, which has none, also under (c) a second plan of the L primes just above 2^60, where a candidate passes with probability
    one half and every cell takes two blocks or more.  Prints us per call: median (min ... max) of --reps groups of --launches calls."""
    import statistics

    L, words = args.primes, args.batch * args.n
    key = bytes(range(32))
    out = torch.empty(L * words, dtype=torch.int64, device="cuda")
    p = out.data_ptr()
    plan.fill_synthetic(p, args.batch, 0, 42, stream)
    draws = [0]      # a nonce is never reused under one key for one kind

    def nonce():
        draws[0] += 1
        return draws[0]

    def fill():
        out.fill_(1)

    def forward():
        plan.forward_range(p, p, args.batch, 0, L, stream)

    wide = None
    if args.kind == "uniform":
        wide = agx.Plan(args.n, _primes_above(1 << 60, args.n, L))

        def uniform():
            plan.sample_uniform(key, nonce(), p, args.batch, 0, 0, L, stream)

        def uniform_above60():
            wide.sample_uniform(key, nonce(), p, args.batch, 0, 0, L, stream)

        todo = [uniform, uniform_above60, fill, forward]
    else:
        def draw(form):
            if args.kind == "ternary":
                plan.sample_ternary(key, nonce(), p, args.batch, 0, 0, L, form, stream)
            else:
                plan.sample_cbd(key, nonce(), args.eta, p, args.batch, 0, 0, L, form, stream)

        def coeff():
            draw(agx.FORM_COEFF)

        def ntt():
            draw(agx.FORM_NTT)

        todo = [coeff, ntt, fill, forward]
    times = _alternate(todo)
    print(f"sample kind={args.kind}{' eta=' + str(args.eta) if args.kind == 'cbd' else ''} n={args.n} L={L} batch={args.batch} bits={args.bits} "
          f"({8 * L * words / 2**20:.0f} MiB written):")
    for name, v in times.items():
        print(f"  {name} {_fmt(v)} us")
    med = {k: statistics.median(v) for k, v in times.items()}
    first = todo[0].__name__
    print("  " + "  ".join(f"{name}/{ref} {med[name] / med[ref]:.3f}" for name in med if name not in ("fill", "forward") for ref in ("fill", "forward")) +
          (f"  ntt/(coeff + forward) {med['ntt'] / (med['coeff'] + med['forward']):.3f}" if "ntt" in med else "") +
          f"  {first}: {med[first] * 1e3 / (L * words):.4f} ns per word")
    if args.report:
        import json

        json.dump({"us": times, "launches": args.launches, "model_bytes": 8.0 * L * words}, open(args.report, "w"))
    if wide is not None:
        wide.close()
    plan.close()


def run_bfvconv():
    """agx_ntt_basis_extend_exact and agx_ntt_basis_extend_mont in coefficient form from the sources [0, S) to the targets [S, S + T) with the auxiliary
    prime S + T, alternating in one process with two yardsticks: agx_ntt_basis_extend (AGX_FORM_COEFF) of the same S sources into the T + 1 primes
    [S, S + T + 1) -- the same matrix work, the auxiliary row included, without the correction -- and a device copy that moves the exact form's model bytes,
    8 (S + 1 + T) per coefficient.  Prints us per call: median (min ... max) of --reps groups of --launches calls."""
    import statistics

    S, T = args.src, args.dst
    words = args.batch * args.n
    basis = plan.basis_aux(0, S, S, T, S + T)
    parent = plan.basis(0, S, S, T + 1)
    # fill_synthetic writes a slab for EVERY prime of the plan: x holds the S source slabs, then T unused ones, then the auxiliary slab at S + T
    x = torch.empty(args.primes * words, dtype=torch.int64, device="cuda")
    out = torch.empty((T + 1) * words, dtype=torch.int64, device="cuda")
    plan.fill_synthetic(x.data_ptr(), args.batch, 0, 42, stream)
    xaux = x.data_ptr() + 8 * (S + T) * words
    half = (S + 1 + T) * words // 2      # a copy reads and writes this many words: together the model's bytes
    c_src, c_dst = (torch.empty(half, dtype=torch.int64, device="cuda") for _ in range(2))

    def exact():
        basis.extend_exact(x.data_ptr(), xaux, out.data_ptr(), args.batch, agx.FORM_COEFF, stream)

    def mont():
        basis.extend_mont(x.data_ptr(), out.data_ptr(), args.batch, agx.FORM_COEFF, stream)

    def extend():
        parent.extend(x.data_ptr(), out.data_ptr(), args.batch, agx.FORM_COEFF, stream)

    def copy():
        c_dst.copy_(c_src)

    todo = [f for name, f in (("exact", exact), ("mont", mont), ("parent", extend), ("copy", copy)) if args.only in ("all", name)]
    times = _alternate(todo)
    model = {"exact": 8.0 * words * (S + 1 + T), "mont": 8.0 * words * (S + T), "extend": 8.0 * words * (S + T + 1), "copy": 16.0 * half}
    print(f"bfvconv n={args.n} S={S} T={T} batch={args.batch} bits={args.bits} launches_ntt_form={basis.aux_info()[2]}:",
          "; ".join(f"{name} {_fmt(t)} us, {model[name] / statistics.median(t) / 1e3:.0f} GB/s of model traffic" for name, t in times.items()))
    if "copy" in times:
        for name in ("exact", "mont", "extend"):
            if name in times:
                print(f"  {name}/copy {statistics.median(times[name]) / statistics.median(times['copy']):.3f}", end="")
        print()
    if "extend" in times:
        for name in ("exact", "mont"):
            if name in times:
                print(f"  {name}/extend {statistics.median(times[name]) / statistics.median(times['extend']):.3f}", end="")
        print()
    if args.report:
        import json

        json.dump({"us": times, "launches": args.launches, "model_bytes": model}, open(args.report, "w"))
    basis.close()
    parent.close()
    plan.close()


def _pointwise_and_add(p, a_ptr, key_rep, acc, tmp, batch, terms, outputs, qcol):
    """step 3 without agx_ntt_inner_product, at its cheapest: terms x outputs agx_ntt_pointwise calls against a key REPLICATED over the batch
    (pointwise cannot broadcast), the products of terms >= 1 added in torch without a reduction (four 60-bit residues fit int64) and one
    remainder per output at the end.  a: [terms][P][batch][n] at a_ptr; key_rep: [terms][outputs][P][batch][n]; acc: [outputs][P][batch][n]"""
    words = p.num_primes * batch * p.n
    for o in range(outputs):
        out = acc[o * words:(o + 1) * words]
        for t in range(terms):
            dst = out if t == 0 else tmp
            p.pointwise(a_ptr + 8 * t * words, key_rep.data_ptr() + 8 * (t * outputs + o) * words, dst.data_ptr(), batch, stream)
            if t:
                out.add_(tmp)
        if terms > 1:
            out.view(p.num_primes, -1).remainder_(qcol)


def run_inner():
    """agx_ntt_inner_product with --terms terms and --outputs outputs over the plan's primes, three ways alternating in one process:
      inner  -- the one call (--bcast: one key frame per prime, bhat_batch = 1);
      copy   -- a device-to-device copy that reads and writes, together, the bytes of the call's traffic model 8 (terms + outputs) per word + the key;
      parent -- _pointwise_and_add above, the key replicated over the batch.
    Prints us per call (median (min ... max) of --reps groups of --launches calls), the model traffic as GB/s, and the ratios."""
    import statistics

    T, O, P, words = args.terms, args.outputs, args.primes, args.primes * args.batch * args.n
    kb = 1 if args.bcast else args.batch
    a = torch.empty(T * words, dtype=torch.int64, device="cuda")
    for t in range(T):
        plan.fill_synthetic(a.data_ptr() + 8 * t * words, args.batch, t * args.batch, 42, stream)
    key_rep = torch.empty(T * O * words, dtype=torch.int64, device="cuda")      # [terms][outputs][P][batch][n]: every frame of a prime the same when --bcast
    for k in range(T * O):
        plan.fill_synthetic(key_rep.data_ptr() + 8 * k * words, args.batch, 0 if args.bcast else (T + k) * args.batch, 43, stream)
    if args.bcast:
        key_rep.view(T * O * P, args.batch, args.n)[:, 1:] = key_rep.view(T * O * P, args.batch, args.n)[:, :1]
    key = key_rep.view(T * O * P, args.batch, args.n)[:, :kb].contiguous().view(-1)      # [terms][outputs][P][kb][n]
    c, acc, tmp = (torch.empty(n_, dtype=torch.int64, device="cuda") for n_ in (O * words, O * words, words))
    qcol = torch.tensor(plan.moduli, dtype=torch.int64, device="cuda")[:, None]
    model = 8.0 * ((T + O) * words + key.numel())
    half = int(model // 16)
    src, dst = (torch.empty(half, dtype=torch.int64, device="cuda") for _ in range(2))
    src.zero_()

    def inner():
        plan.inner_product(a.data_ptr(), key.data_ptr(), c.data_ptr(), args.batch, T, O, kb, stream)

    def copy():
        dst.copy_(src)

    def parent():
        _pointwise_and_add(plan, a.data_ptr(), key_rep, acc, tmp, args.batch, T, O, qcol)

    inner()
    parent()
    torch.cuda.synchronize()
    assert torch.equal(c, acc), "the one call and the pointwise-and-add form differ"
    times = _alternate([f for f in (inner, copy, parent) if args.only in ("all", "both", f.__name__)])
    med = {k: statistics.median(v) for k, v in times.items()}
    head = f"inner n={args.n} P={P} batch={args.batch} terms={T} outputs={O} key={'broadcast' if args.bcast else 'per frame'} bits={args.bits}:"
    parts = [f"{k} {_fmt(v)} us" + (f", {model / med[k] / 1e3:.0f} GB/s of model traffic" if k != "parent" else "") for k, v in times.items()]
    parts += [f"ratio inner/{o} {med['inner'] / med[o]:.3f}" for o in ("copy", "parent") if "inner" in med and o in med]
    print(head, "; ".join(parts))
    if args.report:
        import json

        json.dump({"us": times, "launches": args.launches, "model_bytes": model}, open(args.report, "w"))
    plan.close()


def run_keyswitch():
    """agx_ntt_keyswitch_apply at the shape (--qcount, --pfirst, --pcount, --alpha) on a plan of pfirst + pcount primes, beside the composition of
    public calls a caller had before it: agx_ntt_inverse on a second plan over Q, agx_ntt_basis_extend per digit, step 3 by _pointwise_and_add on a
    third plan over the active primes with the key replicated over the batch, two agx_ntt_basis_mod_down.  Then the stages of the composition one
    by one (step 3 both ways): the split by launch.  us per call, median (min ... max)."""
    import statistics

    Q, pf, pc, alpha, n, B = args.qcount, args.pfirst, args.pcount, args.alpha, args.n, args.batch
    A, slab = Q + pc, args.batch * args.n
    act = list(range(Q)) + list(range(pf, pf + pc))
    psi = [plan.psi(p) for p in range(plan.num_primes)]
    qplan = agx.Plan(n, plan.moduli[:Q], psi=psi[:Q])
    aplan = agx.Plan(n, [plan.moduli[p] for p in act], psi=[psi[p] for p in act])
    ks = plan.keyswitch(Q, pf, pc, alpha)
    digs = [(f, min(alpha, Q - f)) for f in range(0, Q, alpha)]
    D = len(digs)
    ups = [[plan.basis(f, cnt, 0, A)] if pf == Q else [plan.basis(f, cnt, 0, Q), plan.basis(f, cnt, pf, pc)] for f, cnt in digs]
    down = plan.basis(pf, pc, 0, Q)
    chat = torch.empty(plan.num_primes * slab, dtype=torch.int64, device="cuda")      # synthetic residues taken as NTT-form words; slabs [0, Q) are read
    plan.fill_synthetic(chat.data_ptr(), B, 0, 42, stream)
    key_rep = torch.empty(D * 2 * A * slab, dtype=torch.int64, device="cuda")
    for k in range(D * 2):
        aplan.fill_synthetic(key_rep.data_ptr() + 8 * k * A * slab, B, 0, 43 + k, stream)
    kv = key_rep.view(D * 2 * A, B, n)
    kv[:, 1:] = kv[:, :1]
    key = kv[:, 0].contiguous().view(-1)      # [digits][2][A][n]
    out, out2 = (torch.empty(2 * Q * slab, dtype=torch.int64, device="cuda") for _ in range(2))
    scratch = torch.empty(ks.scratch_words(B), dtype=torch.int64, device="cuda")
    coeff, ext, acc, tmp = (torch.empty(k * slab, dtype=torch.int64, device="cuda") for k in (Q, D * A, 2 * A, A))
    qcol = torch.tensor(aplan.moduli, dtype=torch.int64, device="cuda")[:, None]

    def one_call():
        ks.apply(chat.data_ptr(), key.data_ptr(), out.data_ptr(), scratch.data_ptr(), B, stream)

    def inverse():
        qplan.inverse(chat.data_ptr(), coeff.data_ptr(), B, stream)

    def mod_up():
        for d, (f, cnt) in enumerate(digs):
            e = ext.data_ptr() + 8 * d * A * slab
            ups[d][0].extend(coeff.data_ptr() + 8 * f * slab, e, B, agx.FORM_NTT, stream)
            if pf != Q:
                ups[d][1].extend(coeff.data_ptr() + 8 * f * slab, e + 8 * Q * slab, B, agx.FORM_NTT, stream)

    def inner_product():
        aplan.inner_product(ext.data_ptr(), key.data_ptr(), acc.data_ptr(), B, D, 2, 1, stream)

    def pointwise_and_add():
        _pointwise_and_add(aplan, ext.data_ptr(), key_rep, acc, tmp, B, D, 2, qcol)

    def mod_down():
        for o in range(2):
            xq = acc.data_ptr() + 8 * o * A * slab
            down.mod_down(xq, xq + 8 * Q * slab, out2.data_ptr() + 8 * o * Q * slab, xq + 8 * Q * slab, B, stream)

    def composition():
        inverse()
        mod_up()
        pointwise_and_add()
        mod_down()

    one_call()
    composition()
    torch.cuda.synchronize()
    assert torch.equal(out, out2), "the one call and the composition of public calls differ"
    whole = _alternate([one_call, composition])
    stages = _alternate([inverse, mod_up, inner_product, pointwise_and_add])
    inner_product()      # mod_down gives its special slabs up: refill acc before every group by timing it alone, on whatever words it left
    stages.update(_alternate([mod_down]))
    med = {k: statistics.median(v) for k, v in {**whole, **stages}.items()}
    print(f"keyswitch n={n} shape=({Q}, {pf}, {pc}, {alpha}) batch={B} bits={args.bits} launches={ks.info()[5]}: one call {_fmt(whole['one_call'])} us; composition "
          f"{_fmt(whole['composition'])} us; ratio {med['one_call'] / med['composition']:.3f}")
    print("  stages: " + "; ".join(f"{k} {_fmt(v)} us" for k, v in stages.items())
          + f"; sum with inner_product {med['inverse'] + med['mod_up'] + med['inner_product'] + med['mod_down']:.1f} us")
    if args.report:
        import json

        json.dump({"us": {**whole, **stages}, "launches": args.launches, "kernel_launches": ks.info()[5]}, open(args.report, "w"))
    for b in [x for pair in ups for x in pair] + [down]:
        b.close()
    ks.close()
    qplan.close()
    aplan.close()
    plan.close()


def run_hoist():
    """Hoisted rotations at the shape (--qcount, --pfirst, --pcount, --alpha), us per call, median (min ... max), the forms of a line alternating:
      kernel    -- agx_ntt_inner_product_galois (terms = digits, two outputs, broadcast key, over the active primes, g = --galois) beside the plain
                   agx_ntt_inner_product of the same shape and beside the pair it replaces: agx_ntt_automorphism(NTT) over the digits x A slabs into a
                   permuted copy, then agx_ntt_inner_product;
      halves    -- agx_ntt_keyswitch_decompose and one agx_ntt_keyswitch_apply_decomposed alone, beside agx_ntt_keyswitch_apply;
      rotations -- for every R of --rotations: decompose once + R apply_decomposed beside R x (agx_ntt_automorphism on chat + agx_ntt_keyswitch_apply)."""
    import statistics

    Q, pf, pc, alpha, n, B = args.qcount, args.pfirst, args.pcount, args.alpha, args.n, args.batch
    A, slab = Q + pc, args.batch * args.n
    g0 = args.galois % (2 * n)
    act = list(range(Q)) + list(range(pf, pf + pc))
    psi = [plan.psi(p) for p in range(plan.num_primes)]
    qplan = agx.Plan(n, plan.moduli[:Q], psi=psi[:Q])
    aplan = agx.Plan(n, [plan.moduli[p] for p in act], psi=[psi[p] for p in act])
    ks = plan.keyswitch(Q, pf, pc, alpha)
    D = ks.info()[4]
    ext_words, ds_words, as_words = ks.hoisted_words(B)
    chat = torch.empty(plan.num_primes * slab, dtype=torch.int64, device="cuda")      # synthetic residues taken as NTT-form words; slabs [0, Q) are read
    plan.fill_synthetic(chat.data_ptr(), B, 0, 42, stream)
    key = torch.empty(D * 2 * A * n, dtype=torch.int64, device="cuda")      # [digits][2][A][n]
    for k in range(D * 2):
        aplan.fill_synthetic(key.data_ptr() + 8 * k * A * n, 1, k, 43, stream)
    ext, perm = (torch.empty(ext_words, dtype=torch.int64, device="cuda") for _ in range(2))
    rot, dscr, ascr = (torch.empty(w, dtype=torch.int64, device="cuda") for w in (Q * slab, ds_words, as_words))
    acc, acc2 = (torch.empty(2 * A * slab, dtype=torch.int64, device="cuda") for _ in range(2))
    out, out2 = (torch.empty(2 * Q * slab, dtype=torch.int64, device="cuda") for _ in range(2))
    scratch = torch.empty(ks.scratch_words(B), dtype=torch.int64, device="cuda")

    def galois():
        aplan.inner_product_galois(ext.data_ptr(), key.data_ptr(), acc.data_ptr(), B, D, g0, 2, 1, stream)

    def plain():
        aplan.inner_product(ext.data_ptr(), key.data_ptr(), acc2.data_ptr(), B, D, 2, 1, stream)

    def pair():
        aplan.automorphism(ext.data_ptr(), perm.data_ptr(), D * B, g0, agx.FORM_NTT, stream)      # [D][A][B][n]: D A B frames, each permuted alike
        aplan.inner_product(perm.data_ptr(), key.data_ptr(), acc2.data_ptr(), B, D, 2, 1, stream)

    def decompose():
        ks.decompose(chat.data_ptr(), ext.data_ptr(), dscr.data_ptr(), B, stream)

    def apply_decomposed():
        ks.apply_decomposed(ext.data_ptr(), key.data_ptr(), out.data_ptr(), ascr.data_ptr(), B, g0, stream)

    def apply():
        ks.apply(chat.data_ptr(), key.data_ptr(), out2.data_ptr(), scratch.data_ptr(), B, stream)

    decompose()
    galois()
    pair()
    torch.cuda.synchronize()
    assert torch.equal(acc, acc2), "the gathered inner product and automorphism + inner product differ"
    ks.apply_decomposed(ext.data_ptr(), key.data_ptr(), out.data_ptr(), ascr.data_ptr(), B, 1, stream)
    apply()
    torch.cuda.synchronize()
    assert torch.equal(out, out2), "decompose + apply_decomposed(g = 1) and apply differ"
    head = f"hoist n={n} shape=({Q}, {pf}, {pc}, {alpha}) batch={B} bits={args.bits} g={g0}"
    report = {}
    t = _alternate([galois, plain, pair])
    report.update(t)
    med = {k: statistics.median(v) for k, v in t.items()}
    print(f"{head} kernel (terms={D}, outputs=2, A={A}): galois {_fmt(t['galois'])} us; plain {_fmt(t['plain'])} us; automorphism + plain {_fmt(t['pair'])} us; "
          f"ratio galois/plain {med['galois'] / med['plain']:.3f}; galois/pair {med['galois'] / med['pair']:.3f}")
    t = _alternate([decompose, apply_decomposed, apply])
    report.update(t)
    med = {k: statistics.median(v) for k, v in t.items()}
    first, second = ks.hoisted_info()
    print(f"{head} halves (launches {first} + {second}): decompose {_fmt(t['decompose'])} us; apply_decomposed {_fmt(t['apply_decomposed'])} us; apply {_fmt(t['apply'])} us; "
          f"(decompose + apply_decomposed) / apply {(med['decompose'] + med['apply_decomposed']) / med['apply']:.3f}")
    for R in args.rotations:
        gs = [pow(g0, r + 1, 2 * n) for r in range(R)]

        def hoisted():
            decompose()
            for g in gs:
                ks.apply_decomposed(ext.data_ptr(), key.data_ptr(), out.data_ptr(), ascr.data_ptr(), B, g, stream)

        def separate():
            for g in gs:
                qplan.automorphism(chat.data_ptr(), rot.data_ptr(), B, g, agx.FORM_NTT, stream)
                ks.apply(rot.data_ptr(), key.data_ptr(), out2.data_ptr(), scratch.data_ptr(), B, stream)

        t = _alternate([hoisted, separate])
        report.update({f"{k}_{R}": v for k, v in t.items()})
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"{head} rotations R={R}: hoisted {_fmt(t['hoisted'])} us; automorphism + apply each {_fmt(t['separate'])} us; ratio {med['hoisted'] / med['separate']:.3f}")
    if args.report:
        import json

        json.dump({"us": report, "launches": args.launches, "kernel_launches": [first, second]}, open(args.report, "w"))
    ks.close()
    qplan.close()
    aplan.close()
    plan.close()


def run_dhoist():
    """Double-hoisted linear transforms at the shape (--qcount, --pfirst, --pcount, --alpha), us per call, median (min ... max), the forms of a line alternating:
      kernel    -- one agx_ntt_keyswitch_accumulate_decomposed with a one-frame weight, accumulating (g = --galois), beside the same call without the
                   accumulate, beside agx_ntt_inner_product_galois of the same shape (terms = digits, two outputs, broadcast key, over the active primes) and
                   beside a device copy of the accumulating call's model bytes: 8 (digits + 2 + 2 accumulate) per word of a frame per active prime, plus the
                   key and the weight once;
      transform -- for every R of --rotations, out = sum_r w_r o sigma_{g_r}(ct) by two routes on this library, both from chat = c1 and c0:
                   double: decompose, R accumulate_decomposed, ONE keyswitch_mod_down, R mul_add_galois of c0;
                   single: decompose, then per rotation apply_decomposed into a temporary and three mul_add_galois (w o tmp_0, w o tmp_1, w o sigma_g(c0))."""
    import statistics

    Q, pf, pc, alpha, n, B = args.qcount, args.pfirst, args.pcount, args.alpha, args.n, args.batch
    A, slab = Q + pc, args.batch * args.n
    g0 = args.galois % (2 * n)
    act = list(range(Q)) + list(range(pf, pf + pc))
    psi = [plan.psi(p) for p in range(plan.num_primes)]
    aplan = agx.Plan(n, [plan.moduli[p] for p in act], psi=[psi[p] for p in act])
    ks = plan.keyswitch(Q, pf, pc, alpha)
    D = ks.info()[4]
    ext_words, ds_words, as_words = ks.hoisted_words(B)
    R_max = max(args.rotations)
    chat = torch.empty(plan.num_primes * slab, dtype=torch.int64, device="cuda")      # synthetic residues taken as NTT-form words; slabs [0, Q) are c1, and c0 too
    plan.fill_synthetic(chat.data_ptr(), B, 0, 42, stream)
    key = torch.empty(D * 2 * A * n, dtype=torch.int64, device="cuda")      # [digits][2][A][n], one key for every rotation: the time does not depend on its words
    for k in range(D * 2):
        aplan.fill_synthetic(key.data_ptr() + 8 * k * A * n, 1, k, 43, stream)
    weights = torch.empty(R_max * A * n, dtype=torch.int64, device="cuda")      # [R][A][1][n]
    aplan.fill_synthetic(weights.data_ptr(), 1, 0, 44, stream)
    for r in range(1, R_max):
        aplan.fill_synthetic(weights.data_ptr() + 8 * r * A * n, 1, r, 44, stream)
    w_ptr = [weights.data_ptr() + 8 * r * A * n for r in range(R_max)]
    ext = torch.empty(ext_words, dtype=torch.int64, device="cuda")
    dscr, acc, acc2, ascr = (torch.empty(w, dtype=torch.int64, device="cuda") for w in (ds_words, as_words, as_words, as_words))
    out, out2, tmp = (torch.empty(2 * Q * slab, dtype=torch.int64, device="cuda") for _ in range(3))
    model = 8.0 * ((D + 2 + 2) * A * slab + D * 2 * A * n + A * n)
    src, dst = (torch.empty(int(model // 16), dtype=torch.int64, device="cuda") for _ in range(2))
    src.zero_()
    acc.zero_()
    c0 = chat.data_ptr()

    def weighted_acc():
        ks.accumulate_decomposed(ext.data_ptr(), key.data_ptr(), acc.data_ptr(), B, g0, w_ptr[0], 1, True, stream)

    def weighted():
        ks.accumulate_decomposed(ext.data_ptr(), key.data_ptr(), acc2.data_ptr(), B, g0, w_ptr[0], 1, False, stream)

    def galois():
        aplan.inner_product_galois(ext.data_ptr(), key.data_ptr(), acc2.data_ptr(), B, D, g0, 2, 1, stream)

    def copy():
        dst.copy_(src)

    ks.decompose(chat.data_ptr(), ext.data_ptr(), dscr.data_ptr(), B, stream)
    # accumulate(no weight, nothing accumulated) + mod_down is apply_decomposed
    ks.accumulate_decomposed(ext.data_ptr(), key.data_ptr(), acc2.data_ptr(), B, g0, stream=stream)
    ks.mod_down(acc2.data_ptr(), out.data_ptr(), B, stream)
    ks.apply_decomposed(ext.data_ptr(), key.data_ptr(), out2.data_ptr(), ascr.data_ptr(), B, g0, stream)
    torch.cuda.synchronize()
    assert torch.equal(out, out2), "accumulate_decomposed + keyswitch_mod_down and apply_decomposed differ"
    head = f"dhoist n={n} shape=({Q}, {pf}, {pc}, {alpha}) batch={B} bits={args.bits} g={g0}"
    report = {}
    t = _alternate([weighted_acc, weighted, galois, copy])
    report.update(t)
    med = {k: statistics.median(v) for k, v in t.items()}
    print(f"{head} kernel (terms={D}, A={A}, model {model / 1e6:.1f} MB): weighted+accumulate {_fmt(t['weighted_acc'])} us; weighted {_fmt(t['weighted'])} us; "
          f"galois {_fmt(t['galois'])} us; copy {_fmt(t['copy'])} us; ratio weighted_acc/copy {med['weighted_acc'] / med['copy']:.3f}; "
          f"weighted_acc/galois {med['weighted_acc'] / med['galois']:.3f}; weighted/galois {med['weighted'] / med['galois']:.3f}")
    down = ks.hoisted_info()[1] - 1
    for R in args.rotations:
        gs = [pow(g0, r + 1, 2 * n) for r in range(R)]

        def double():
            ks.decompose(chat.data_ptr(), ext.data_ptr(), dscr.data_ptr(), B, stream)
            for r, g in enumerate(gs):
                ks.accumulate_decomposed(ext.data_ptr(), key.data_ptr(), acc.data_ptr(), B, g, w_ptr[r], 1, r > 0, stream)
            ks.mod_down(acc.data_ptr(), out.data_ptr(), B, stream)
            for r, g in enumerate(gs):
                plan.mul_add_galois(w_ptr[r], c0, out.data_ptr(), B, g, 1, True, 0, Q, stream)

        def single():
            ks.decompose(chat.data_ptr(), ext.data_ptr(), dscr.data_ptr(), B, stream)
            for r, g in enumerate(gs):
                ks.apply_decomposed(ext.data_ptr(), key.data_ptr(), tmp.data_ptr(), ascr.data_ptr(), B, g, stream)
                plan.mul_add_galois(w_ptr[r], tmp.data_ptr(), out2.data_ptr(), B, 1, 1, r > 0, 0, Q, stream)
                plan.mul_add_galois(w_ptr[r], tmp.data_ptr() + 8 * Q * slab, out2.data_ptr() + 8 * Q * slab, B, 1, 1, r > 0, 0, Q, stream)
                plan.mul_add_galois(w_ptr[r], c0, out2.data_ptr(), B, g, 1, True, 0, Q, stream)

        t = _alternate([double, single])
        report.update({f"{k}_{R}": v for k, v in t.items()})
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"{head} transform R={R} (ModDown launches {down} against {R * down}): double-hoisted {_fmt(t['double'])} us; single-hoisted {_fmt(t['single'])} us; "
              f"ratio double/single {med['double'] / med['single']:.3f}")
    if args.report:
        import json

        json.dump({"us": report, "launches": args.launches, "model_bytes": model}, open(args.report, "w"))
    ks.close()
    aplan.close()
    plan.close()


def run_ring():
    """One ring call (--kind add, sub, negate, add_galois or tensor) on the primes [--first, --first + --count) of a plan of --primes primes, alternating
    in one process with
      copy   -- a device-to-device copy that reads and writes, together, the call's model bytes: 24 / 24 / 16 / 24 / 56 per word;
      parent -- what a caller had before: tensor: four agx_ntt_pointwise launches into four buffers on a second plan over the range's primes (the
                cross term's add not included); add_galois: agx_ntt_automorphism into a copy on that plan, then a torch add and remainder.
    Prints us per call (median (min ... max) of --reps groups of --launches calls), the model traffic as GB/s, and the ratios."""
    import statistics

    kind, first, count = args.kind, args.first, args.count
    words = count * args.batch * args.n
    k_in, k_out = (2, 3) if kind == "tensor" else (1, 1)
    moduli = plan.moduli[first:first + count]
    qplan = agx.Plan(args.n, moduli)      # only to fill the operands and for the parent's calls, which take all primes of their plan
    a, b = (torch.empty(k_in * words, dtype=torch.int64, device="cuda") for _ in range(2))
    for k in range(k_in):
        qplan.fill_synthetic(a.data_ptr() + 8 * k * words, args.batch, k * args.batch, 42, stream)
        qplan.fill_synthetic(b.data_ptr() + 8 * k * words, args.batch, (2 + k) * args.batch, 43, stream)
    c, ref, tmp = (torch.empty(k_out * words, dtype=torch.int64, device="cuda") for _ in range(3))
    extra = torch.empty(words, dtype=torch.int64, device="cuda")
    qcol = torch.tensor(moduli, dtype=torch.int64, device="cuda")[:, None]
    g = args.galois % (2 * args.n)
    model = 8.0 * words * {"add": 3, "sub": 3, "negate": 2, "add_galois": 3, "tensor": 7}[kind]
    half = int(model // 16)
    src, dst = (torch.empty(half, dtype=torch.int64, device="cuda") for _ in range(2))
    src.zero_()
    pa, pb, pc = a.data_ptr(), b.data_ptr(), c.data_ptr()

    def ring():
        if kind == "add":
            plan.add(pa, pb, pc, args.batch, first, count, stream)
        elif kind == "sub":
            plan.sub(pa, pb, pc, args.batch, first, count, stream)
        elif kind == "negate":
            plan.negate(pa, pc, args.batch, first, count, stream)
        elif kind == "add_galois":
            plan.add_galois(pa, pb, pc, args.batch, g, first, count, stream)
        else:
            plan.tensor(pa, pb, pc, args.batch, first, count, stream)

    def copy():
        dst.copy_(src)

    def parent():
        if kind == "tensor":      # c_0, the two halves of c_1, c_2
            for i, (x, y, out) in enumerate(((0, 0, ref), (0, 1, tmp), (1, 0, extra), (1, 1, ref))):
                qplan.pointwise(pa + 8 * x * words, pb + 8 * y * words, out.data_ptr() + (16 * words if i == 3 else 0), args.batch, stream)
        else:
            qplan.automorphism(pb, tmp.data_ptr(), args.batch, g, agx.FORM_NTT, stream)
            torch.add(a, tmp, out=ref)
            ref.view(count, -1).remainder_(qcol)

    todo = [ring, copy] + ([parent] if kind in ("tensor", "add_galois") else [])
    ring()
    torch.cuda.synchronize()
    av, bv = a.view(k_in, count, -1), b.view(k_in, count, -1)
    if kind == "tensor":
        parent()
        torch.cuda.synchronize()
        cv, rv = c.view(3, count, -1), ref.view(3, count, -1)
        assert torch.equal(cv[0], rv[0]) and torch.equal(cv[2], rv[2]), "c_0 or c_2 differs from agx_ntt_pointwise"
        assert torch.equal(cv[1], (tmp[:words].view(count, -1) + extra.view(count, -1)) % qcol), "c_1 differs from the sum of the two pointwise products"
    elif kind == "add_galois":
        parent()
        torch.cuda.synchronize()
        assert torch.equal(c, ref), "the one call and automorphism-plus-add differ"
    else:
        want = {"add": (av[0] + bv[0]) % qcol, "sub": (av[0] - bv[0]) % qcol, "negate": (-av[0]) % qcol}[kind]
        assert torch.equal(c.view(count, -1), want), "the call's words differ from torch's"
    times = _alternate([f for f in todo if args.only in ("all", "both", f.__name__)])
    med = {k: statistics.median(v) for k, v in times.items()}
    head = f"ring {kind} n={args.n} P={args.primes} range=({first}, {count}) batch={args.batch} bits={args.bits}" + (f" g={g}" if kind == "add_galois" else "") + ":"
    parts = [f"{k} {_fmt(v)} us" + (f", {model / med[k] / 1e3:.0f} GB/s of model traffic" if k != "parent" else "") for k, v in times.items()]
    parts += [f"ratio ring/{o} {med['ring'] / med[o]:.3f}" for o in ("copy", "parent") if "ring" in med and o in med]
    print(head, "; ".join(parts))
    if args.report:
        import json

        json.dump({"us": times, "launches": args.launches, "model_bytes": model}, open(args.report, "w"))
    qplan.close()
    plan.close()


if args.op == "ring":
    run_ring()
    sys.exit(0)
if args.op == "inner":
    run_inner()
    sys.exit(0)
if args.op == "hoist":
    run_hoist()
    sys.exit(0)
if args.op == "dhoist":
    run_dhoist()
    sys.exit(0)
if args.op == "keyswitch":
    run_keyswitch()
    sys.exit(0)
if args.op == "auto":
    run_auto()
    sys.exit(0)
if args.op == "moddown":
    run_moddown()
    sys.exit(0)
if args.op == "extend":
    run_extend()
    sys.exit(0)
if args.op == "bfvconv":
    run_bfvconv()
    sys.exit(0)
if args.op == "quotient":
    run_quotient()
    sys.exit(0)
if args.op == "plain":
    run_plain()
    sys.exit(0)
if args.op == "sample":
    run_sample()
    sys.exit(0)
if args.op == "ckks":
    run_ckks()
    sys.exit(0)
if args.op == "batch":
    run_batch()
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
