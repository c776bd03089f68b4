#!/usr/bin/env python3
"""Is the device code of a set of .hip files what another set's was?  Per .amdhsa_kernel symbol, the text from the symbol's label to
the .end_amdhsa_kernel of its descriptor block is compared (profiles/r13/leaf_plan_refactor.txt is this tool's output).
    hipcc <the Makefile's flags> --offload-device-only -S old.hip -o old.s      (and the same for every new file)
    tools/compare_kernel_asm.py old.s [old2.s ...] -- new_a.s [new_b.s ...]
Two things in a kernel's text depend on where the function stands in its file, not on its code, and are normalised: the function's
ordinal in local labels (.LBB<ordinal>_<block>, .Lfunc_end<ordinal>, "BB<ordinal>_<block>" in comments) and the padding between such
a label and the comment on its line.  A kernel that several files of a side hold must be the same text in all of them.  Exit status 1
if the symbol sets differ or any kernel does."""
import re, sys


def kernels(path):
    text = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        i = text.index("\n" + name + ":")
        j = text.index(".end_amdhsa_kernel", text.index(".amdhsa_kernel " + name, i))
        body = re.sub(r"BB\d+_(\d+)", r"BB#_\1", text[i:j])
        body = re.sub(r"(BB#_\d+:) +;", r"\1 ;", body)
        out[name] = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1#", body)
    return out


def side(paths):
    merged, where = {}, {}
    for p in paths:
        for name, body in kernels(p).items():
            if name in merged and merged[name] != body:
                sys.exit(f"{name} differs between {where[name][0]} and {p}")
            merged[name] = body
            where.setdefault(name, []).append(p)
    return merged, where


args = sys.argv[1:]
old, _ = side(args[:args.index("--")])
new, where = side(args[args.index("--") + 1:])
print(f"old: {len(old)} kernels; new: {len(new)} kernels; symbol sets equal: {set(old) == set(new)}")
bad = set(old) != set(new)
for name in sorted(old):
    same = new.get(name) == old[name]
    bad |= not same
    print(("identical  " if same else "DIFFERS    ") + ",".join(where.get(name, ["MISSING"])) + "  " + name)
for name in sorted(set(new) - set(old)):
    print("EXTRA      " + name)
sys.exit(1 if bad else 0)
