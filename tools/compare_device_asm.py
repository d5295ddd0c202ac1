#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device assembly of two builds of csrc/ (is a host-side change really host-side only?).

Compile every device unit of both trees to assembly, product flags and again with -DAGX_DIAG (plus reg_diag.hip), e.g.
    hipcc <the Makefile's HIPFLAGS without --offload-compress> --cuda-device-only -S -o OLD/reg_s1024.prod.s old/csrc/reg_s1024.hip
then  python tools/compare_device_asm.py OLD NEW  splits each <unit>.s per kernel symbol (label to the resource block behind
.end_amdhsa_kernel) and compares by mangled name.  The function index in local labels and loop comments (.LBB<k>_, .Lfunc_end<k>, .Ltmp<k>,
Header=BB<k>_, "Child Loop BB<k>_" / "Parent Loop BB<k>_") is normalised: it shifts when an earlier kernel of the unit disappears or a new one is emitted
ahead of it.  Exit status 0: every kernel of NEW is textually identical to OLD's (so are its registers, scratch, LDS and occupancy); kernels only in OLD
are listed.  A change that adds kernels exits 1 on purpose; its RESULT line says apart how many kernels of OLD are missing or different (what must be 0
for "the old kernels are untouched") and how many are new."""
import glob
import os
import re
import sys


def kernels(path):
    txt = open(path).read().split("\n")
    out = {}
    for name in (m.group(1) for l in txt for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m):
        start = next(i for i, l in enumerate(txt) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(txt)) if txt[i].strip() == ".end_amdhsa_kernel")
        while end + 1 < len(txt) and not re.match(r"\t\.(protected|section|amdgpu_metadata|p2alignl|ident|weak|globl)\b|\s*$", txt[end + 1]):
            end += 1      # the .set block of resource counts behind the descriptor
        out[name] = re.sub(r"(\.LBB|\.Lfunc_end|\.Ltmp|Header=BB|Loop BB)\d+", r"\1#", "\n".join(txt[start:end + 1]))
    return out


def main(old, new):
    bad = changed = 0
    for pa in sorted(glob.glob(os.path.join(old, "*.s"))):
        unit = os.path.basename(pa)
        ka, kb = kernels(pa), kernels(os.path.join(new, unit))
        differ = [n for n in kb if n not in ka or ka[n] != kb[n]]
        bad += len(differ)
        changed += sum(n in ka for n in differ) + sum(n not in kb for n in ka)
        print(f"{unit}: {len(ka)} -> {len(kb)} kernels, {len(kb) - len(differ)} identical, {len(differ)} new or different")
        for n in differ:
            print("   DIFFERENT" if n in ka else "   NEW", n)
        for n in ka:
            if n not in kb:
                print("   only in OLD:", n, f"({ka[n].count(chr(10))} lines)")
    print("RESULT:", "device code unchanged" if bad == 0 else f"{bad} kernels new or different")
    if bad:
        print("RESULT:", f"{changed} kernels of OLD missing or different" + ("" if changed else ": every kernel of OLD is present and textually identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
