#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device assembly of two builds of csrc/ (is a host-side change really host-side only?).

Compile every device unit of both trees to assembly, product flags and again with -DAGX_DIAG (plus reg_diag.hip), e.g.
    hipcc <the Makefile's HIPFLAGS without --offload-compress> --cuda-device-only -S -o OLD/reg_s1024.prod.s old/csrc/reg_s1024.hip
then  python tools/compare_device_asm.py OLD NEW [RENAMES]  splits each <unit>.s per kernel symbol (label to the resource block behind
.end_amdhsa_kernel) and compares by mangled name.  The function index in local labels and loop comments (.LBB<k>_, .Lfunc_end<k>, .Ltmp<k>,
Header=BB<k>_, "Child Loop BB<k>_" / "Parent Loop BB<k>_") is normalised: it shifts when an earlier kernel of the unit disappears or a new one is emitted
ahead of it (so is the padding between a label and its comment, which follows the index's width).  Exit status 0: every kernel of NEW is textually identical to OLD's (so are its registers, scratch, LDS and occupancy); kernels only in OLD
are listed.  A change that adds kernels exits 1 on purpose; its RESULT line says apart how many kernels of OLD are missing or different (what must be 0
for "the old kernels are untouched") and how many are new.

RENAMES (optional; without it nothing below applies) is a file of `old-symbol new-symbol` pairs, one per line (blank lines and lines that start with # are
skipped), for a change that renames kernels: each old symbol of OLD, and every occurrence of it in the kernel's own text, is replaced by the new one before
the comparison.  A renamed kernel that is then identical counts as identical and is listed as `renamed, identical`; the RESULT line gives their number."""
import glob
import os
import re
import sys


def kernels(path, renames={}):
    txt = open(path).read().split("\n")
    out = {}
    for name in (m.group(1) for l in txt for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m):
        start = next(i for i, l in enumerate(txt) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(txt)) if txt[i].strip() == ".end_amdhsa_kernel")
        while end + 1 < len(txt) and not re.match(r"\t\.(protected|section|amdgpu_metadata|p2alignl|ident|weak|globl)\b|\s*$", txt[end + 1]):
            end += 1      # the .set block of resource counts behind the descriptor
        body = re.sub(r"(\.LBB|\.Lfunc_end|\.Ltmp|Header=BB|Loop BB)\d+", r"\1#", "\n".join(txt[start:end + 1]))
        body = re.sub(r"(?m)^(\.LBB#_\d+:)[ \t]+;", r"\1 ;", body)      # a label's comment is padded to a column: the padding shrinks when the index gains a digit
        new = renames.get(name, name)
        out[new] = re.sub(r"(?<![\w$.])" + re.escape(name) + r"(?![\w$])", new, body) if new != name else body
    return out


def read_renames(path):
    pairs = [l.split() for l in open(path) if l.strip() and not l.startswith("#")]
    bad = [p for p in pairs if len(p) != 2]
    if bad:
        sys.exit(f"{path}: not an `old-symbol new-symbol` pair: {' '.join(bad[0])}")
    return dict(pairs)


def main(old, new, renames={}):
    bad = changed = renamed = 0
    new_names = {v: k for k, v in renames.items()}
    for pa in sorted(glob.glob(os.path.join(old, "*.s"))):
        unit = os.path.basename(pa)
        ka, kb = kernels(pa, renames), kernels(os.path.join(new, unit))
        differ = [n for n in kb if n not in ka or ka[n] != kb[n]]
        moved = [n for n in kb if n in new_names and n not in differ]
        bad += len(differ)
        renamed += len(moved)
        changed += sum(n in ka for n in differ) + sum(n not in kb for n in ka)
        print(f"{unit}: {len(ka)} -> {len(kb)} kernels, {len(kb) - len(differ)} identical" + (f" ({len(moved)} of them renamed)" if moved else "") +
              f", {len(differ)} new or different")
        for n in moved:
            print("   renamed, identical:", new_names[n], "->", n)
        for n in differ:
            print("   DIFFERENT" if n in ka else "   NEW", n)
        for n in ka:
            if n not in kb:
                print("   only in OLD:", n, f"({ka[n].count(chr(10))} lines)")
    print("RESULT:", ("device code unchanged" + (f", {renamed} kernels renamed and identical" if renames else "")) if bad == 0 else f"{bad} kernels new or different")
    if bad:
        print("RESULT:", f"{changed} kernels of OLD missing or different" + ("" if changed else ": every kernel of OLD is present and textually identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], read_renames(sys.argv[3]) if len(sys.argv) > 3 else {}))
