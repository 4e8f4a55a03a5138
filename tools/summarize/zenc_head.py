#!/usr/bin/env python3
"""The head of run() (HEVM::plan_zero_encrypt: the zero-encryptions of every opcode-10 item, before the first plan step) from a rocprofv3
kernel trace of a process that calls run() several times:
    python3 tools/summarize/zenc_head.py kernel_trace.csv
A run ends with bump_epoch_kernel.  A head chunk starts with its sampler kernel (sample_enc_batch_kernel / sample_zenc_batch_kernel) and
ends with the first f_frows_final_kernel / f_frows_zenc_final_kernel after it; the head lasts from the first chunk's first kernel start to the last chunk's last kernel
end.  Prints that per run, and each head kernel's calls per run and mean duration over the runs after the first (the warm-up)."""
import csv
import re
import sys
from collections import defaultdict

SAMPLERS = ("sample_enc_batch_kernel", "sample_zenc_batch_kernel")


def short(n):
    return re.sub(r"\(.*", "", n).replace("void dacapo::", "").replace("dacapo::", "")


def main():
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in csv.DictReader(open(sys.argv[1])))
    runs, cur = [], []
    for e in ev:
        cur.append(e)
        if e[2].startswith("bump_epoch_kernel"):
            runs.append(cur)
            cur = []
    heads, stats = [], defaultdict(list)
    for k, run in enumerate(runs):
        first = [i for i, e in enumerate(run) if e[2].startswith(SAMPLERS)]
        if not first:
            continue
        hi = next(i for i in range(first[-1], len(run)) if run[i][2].startswith(("f_frows_final_kernel", "f_frows_zenc_final_kernel")))
        head = run[first[0] : hi + 1]
        span = (max(e[1] for e in head) - head[0][0]) / 1e3
        busy = sum(e[1] - e[0] for e in head) / 1e3
        whole = (run[-1][1] - run[0][0]) / 1e3
        heads.append((span, busy, whole, len(first), len(head)))
        if k:
            per_run = defaultdict(list)
            for e in head:
                per_run[e[2]].append((e[1] - e[0]) / 1e3)
            for n, d in per_run.items():
                stats[n].append(d)
    for k, (span, busy, whole, chunks, n) in enumerate(heads):
        print(f"run {k}: head {span:9.1f} us first start .. last end ({busy:9.1f} us of kernel time, {chunks} chunks, {n} launches)   "
              f"run() first start .. last end {whole / 1e3:8.3f} ms")
    print("head kernels, runs after the first: calls per run, mean us per call, us per run")
    for n, runs_d in sorted(stats.items(), key=lambda kv: -sum(map(sum, kv[1]))):
        calls = sum(len(d) for d in runs_d) / len(runs_d)
        tot = sum(map(sum, runs_d)) / len(runs_d)
        print(f"  {n[:100]:100s} {calls:6.1f} {tot / calls:9.1f} {tot:9.1f}")


if __name__ == "__main__":
    main()
