#!/usr/bin/env python3
"""The kernels option ks_fold_add is about, from a rocprofv3 --kernel-trace of tools/legs/headline_only.py: for the LAST run() of the trace
(bump_epoch_kernel ends every run) the wall time, kernel count, summed kernel time, and per kernel -- every n-ary sum kernel (b_sum*), the
rotations' fused middle (f_ks_frows_mac_kernel<.., 0, ..>) and the rotations' last kernels -- launches, mean and total microseconds.
usage: python tools/summarize/fold_add_trace.py <kernel_trace.csv | results.db> [label]"""
import collections
import csv
import re
import sqlite3
import sys


def events(path):
    if path.endswith(".db"):  # rocprofv3's rocpd output: the `kernels` view
        con = sqlite3.connect(path)
        return [(s, e, n) for s, e, n in con.execute("select start, end, name from kernels")]
    with open(path) as f:
        return [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)]


def short(name):
    return re.sub(r"\(.*", "", name).replace("void dacapo::", "").replace("dacapo::", "")


def main():
    ev = sorted((s, e, short(n)) for s, e, n in events(sys.argv[1]))
    label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
    ends = [i for i, e in enumerate(ev) if e[2].startswith("bump_epoch_kernel")]
    run = ev[ends[-2] + 1:ends[-1] + 1] if len(ends) >= 2 else ev
    busy = sum(e[1] - e[0] for e in run)
    print(f"-- {label}")
    print(f"last run(): {len(run)} kernels, wall {(run[-1][1] - run[0][0]) / 1e6:.2f} ms, kernel time {busy / 1e6:.2f} ms")
    per = collections.defaultdict(lambda: [0, 0])
    for s, e, n in run:
        per[n][0] += 1
        per[n][1] += e - s
    wanted = lambda n: n.startswith("b_sum") or re.match(r"f_ks_frows_mac_kernel<\d+, \d+, 0,", n) or re.match(r"f_frows_final(_cont)?_kernel<\d+, \d+, 0[,>]", n)
    print(f"{'kernel':52s} {'calls':>6s} {'avg_us':>8s} {'total_us':>10s}")
    tot = collections.defaultdict(lambda: [0, 0])
    for n, (k, t) in sorted(per.items(), key=lambda kv: kv[0]):
        if not wanted(n):
            continue
        print(f"{n[:52]:52s} {k:6d} {t / k / 1e3:8.2f} {t / 1e3:10.1f}")
        g = "b_sum*" if n.startswith("b_sum") else "f_ks_frows_mac_kernel<.., 0, ..>" if n.startswith("f_ks") else "rotation last kernels"
        tot[g][0] += k
        tot[g][1] += t
    for g, (k, t) in tot.items():
        print(f"{'total ' + g:52s} {k:6d} {t / max(k, 1) / 1e3:8.2f} {t / 1e3:10.1f}")


if __name__ == "__main__":
    main()
