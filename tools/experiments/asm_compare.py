#!/usr/bin/env python3
"""Per-kernel comparison of two directories of `hipcc -S --cuda-device-only` listings of the same sources (development aid; what
profiles/ks_mac_regs.txt was made with).  A kernel is the text between its label and its .Lfunc_end; comments, .file / .loc / .ident
directives and the numbers of local labels (they count the functions before it) are ignored.
    for f in fused_ks hoist_ks ...; do hipcc <the Makefile's CXXFLAGS> [-DDC_GENERIC_WIDTH=1] -S --cuda-device-only dacapo_amd/csrc/$f.hip -o DIR/$f[.gw].s; done
    python tools/experiments/asm_compare.py PARENT_DIR BRANCH_DIR                    # per file: kernels, identical, the ones that differ
    python tools/experiments/asm_compare.py PARENT_DIR BRANCH_DIR --table 'regex'    # per kernel: vgpr sgpr spills scratch lds, before | after"""
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
    body = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", s, re.M | re.S):
        lines = [l for l in m.group(2).split("\n") if not re.match(r"\s*(\.file|\.loc|\.ident|\.cfi|;\s*%bb|\s*$)", l)]
        lines = [re.sub(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+_?", r".L\1N_", re.sub(r"\s*;.*$", "", l)) for l in lines]
        body[m.group(1)] = [l for l in lines if l.strip()]
    meta = {r[2]: dict(lds=int(r[1]), scratch=int(r[3]), sgpr=int(r[4]), vgpr=int(r[6]), spills=int(r[5]) + int(r[7])) for r in META.findall(s)}
    return body, meta


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(.*", "", x).replace("void dacapo::", "").replace("dacapo::", "") for x in out]


parent, branch = sys.argv[1], sys.argv[2]
table = sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "--table" else None
for f in sorted(glob.glob(os.path.join(branch, "*.s"))):
    base = os.path.basename(f)
    kp, mp = kernels(os.path.join(parent, base))
    kb, mb = kernels(f)
    names = sorted(set(kp) | set(kb))
    dn = dict(zip(names, demangle(names)))
    same = {n for n in names if n in kp and n in kb and kp[n] == kb[n]}
    if not table:
        print(f"{base}: {len(names)} kernels, {len(same)} identical, {len(names) - len(same)} differ or are in one tree only")
        for n in names:
            if n not in same:
                print(f"    {dn[n]}" + ("" if n in kp and n in kb else "  (one tree only)"))
        continue
    for n in names:
        if re.search(table, dn[n]) and n in mp and n in mb:
            a, b = mp[n], mb[n]
            print(f"{base[:-2]:14s} {dn[n]:38s} | {a['vgpr']:4d} {a['sgpr']:4d} {a['spills']:2d} {a['scratch']:3d} {a['lds']:6d} "
                  f"| {b['vgpr']:4d} {b['sgpr']:4d} {b['spills']:2d} {b['scratch']:3d} {b['lds']:6d} | {'identical' if n in same else 'differs'}")
