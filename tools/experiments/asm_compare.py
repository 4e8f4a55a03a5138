#!/usr/bin/env python3
"""Per-kernel comparison of two directories of `hipcc -S --cuda-device-only` listings of the same sources (development aid; what
profiles/ks_mac_regs.txt was made with).  A kernel is the text between its label and its .Lfunc_end; comments, .file / .loc / .ident
directives, the numbers of local labels (they count the functions before it), the kernel's own name and the size of its argument block
(.amdhsa_kernarg_size: a parameter that the code never reads changes nothing else) are ignored.  Identical kernels whose argument blocks differ in size are counted in a note.
    for f in fused_ks hoist_ks ...; do hipcc <the Makefile's CXXFLAGS> [-DDC_GENERIC_WIDTH=1] -S --cuda-device-only dacapo_amd/csrc/$f.hip -o DIR/$f[.gw].s; done
    python tools/experiments/asm_compare.py PARENT_DIR BRANCH_DIR                    # per file: kernels, identical, the ones that differ
    python tools/experiments/asm_compare.py PARENT_DIR BRANCH_DIR --table 'regex'    # per kernel: vgpr sgpr spills scratch lds, before | after
Kernels are paired by name and template arguments (c++filt, the argument list dropped, so a kernel that gained or lost a parameter still
pairs).  Where a name or its template arguments changed, --rename 'REGEX=REPLACEMENT' (repeatable, applied in order to the parent's names) says
which parent kernel a branch kernel is compared with, e.g. --rename 'f_old_kernel<(.*)>=f_new_kernel<\\1, true>'."""
import glob
import os
import re
import subprocess
import sys

META = re.compile(r"- \.agpr_count:\s+(\d+)(?:.*\n)*?\s+\.group_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.name:\s+(\S+)(?:.*\n)*?"
                  r"\s+\.private_segment_fixed_size:\s+(\d+)(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)(?:.*\n)*?"
                  r"\s+\.vgpr_count:\s+(\d+)(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)")


def kernels(path):
    s = open(path).read()
    body, karg = {}, {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", s, re.M | re.S):
        karg[m.group(1)] = (re.findall(r"\.amdhsa_kernarg_size\s+(\d+)", m.group(2)) or ["?"])[0]
        lines = [l for l in m.group(2).split("\n") if not re.match(r"\s*(\.file|\.loc|\.ident|\.cfi|\.amdhsa_kernarg_size|;\s*%bb|\s*$)", l)]
        lines = [re.sub(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+_?", r".L\1N_", re.sub(r"\s*;.*$", "", l)) for l in lines]
        body[m.group(1)] = [l.replace(m.group(1), "KERNEL") for l in lines if l.strip()]  # (its own name: a renamed kernel still pairs)
    meta = {r[2]: dict(lds=int(r[1]), scratch=int(r[3]), sgpr=int(r[4]), vgpr=int(r[6]), spills=int(r[5]) + int(r[7])) for r in META.findall(s)}
    return body, meta, karg


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(.*", "", x).replace("void dacapo::", "").replace("dacapo::", "") for x in out]


def keyed(path, renames=()):
    """{kernel name with its template arguments, without the argument list: (body, resources, argument-block size)}; renames = [(regex, replacement)]"""
    body, meta, karg = kernels(path)
    out = {}
    for n, d in zip(body, demangle(list(body))):
        for old, new in renames:
            d = re.sub(old, new, d)
        assert d not in out, d
        out[d] = (body[n], meta.get(n), karg[n])
    return out


args = sys.argv[1:]
table, renames = None, []
if len(args) < 2 or len(args) % 2:
    sys.exit(__doc__)
while len(args) > 2:
    opt, val = args[-2:]
    args = args[:-2]
    if opt == "--table":
        table = val
    elif opt == "--rename":
        renames.insert(0, tuple(val.split("=", 1)))
    else:
        sys.exit(__doc__)
parent, branch = args
for f in sorted(glob.glob(os.path.join(branch, "*.s"))):
    base = os.path.basename(f)
    kp, kb = keyed(os.path.join(parent, base), renames), keyed(f)
    names = sorted(set(kp) | set(kb))
    same = {n for n in names if n in kp and n in kb and kp[n][0] == kb[n][0]}
    if not table:
        print(f"{base}: {len(names)} kernels, {len(same)} identical, {len(names) - len(same)} differ or are in one tree only")
        for n in names:
            if n not in same:
                print(f"    {n}" + ("" if n in kp and n in kb else "  (one tree only)"))
        resized = [n for n in sorted(same) if kp[n][2] != kb[n][2]]  # (the comparison ignores the size: say so where it differs)
        if resized:
            print(f"    note: {len(resized)} of the identical kernels have another argument-block size, e.g. {resized[0]}: {kp[resized[0]][2]} -> {kb[resized[0]][2]} bytes")
        continue
    for n in names:
        if re.search(table, n) and n in kp and n in kb and kp[n][1] and kb[n][1]:
            a, b = kp[n][1], kb[n][1]
            print(f"{base[:-2]:14s} {n:38s} | {a['vgpr']:4d} {a['sgpr']:4d} {a['spills']:2d} {a['scratch']:3d} {a['lds']:6d} "
                  f"| {b['vgpr']:4d} {b['sgpr']:4d} {b['spills']:2d} {b['scratch']:3d} {b['lds']:6d} | {'identical' if n in same else 'differs'}")
