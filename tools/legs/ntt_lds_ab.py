#!/usr/bin/env python3
"""The single-launch LDS-resident NTT (csrc/ntt_lds.hip, dc_ntt_variant 1) against the two-launch tiles (variant 0, the parent's unchanged
code) on the rings it serves, in ONE process: per ring, direction and limb count the windows 0 / 1 / 0 alternate under HIP events.
A gain counts only if it is negative and larger than five times the 0/0 spread (the rule of profiles/plan_levels_ab.txt).
    python tools/legs/ntt_lds_ab.py [--out profiles/ntt_lds_ab.txt] [--rounds 3]
Each launch is enqueued from Python right behind the previous one on the null stream, as a caller of dc_ntt_forward does: a window's time
per launch includes whatever the dependent launches of that variant cost."""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from dacapo_amd import lowlevel as ll  # noqa: E402

CASES = {14: [1, 13, 26, 169, 4096], 13: [1, 26, 4096], 12: [1, 26, 4096]}  # 2^14: BASELINE workload 1's counts
K = 3


def window(L, ctx, buf, count, inverse, variant, iters, ev):
    for _ in range(3):
        ctx.ntt(buf, count, inverse=inverse, prime_base=0, prime_period=K, variant=variant)
    L.dc_event_record(ev[0], None)
    for _ in range(iters):
        ctx.ntt(buf, count, inverse=inverse, prime_base=0, prime_period=K, variant=variant)
    L.dc_event_record(ev[1], None)
    return L.dc_event_elapsed_ms(ev[0], ev[1]) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ntt_lds_ab.txt"))
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    L = ll.lib()
    ev = (L.dc_event_create(), L.dc_event_create())
    lines = ["Single-launch LDS-resident NTT (ntt_lds_kernel, variant 1) against the two-launch tiles (variant 0 = the parent's code), one MI355X,",
             f"one process; us per launch, mean of {a.rounds} rounds of the windows 0 / 1 / 0; per limb = us per launch / limbs.", ""]
    passes = {}
    for logN, counts in CASES.items():
        ctx = ll.Context(logN, K)
        N = ctx.N
        # same results first, at the sizes timed: 26 limbs, both directions
        q = np.array([ctx.primes[b % K] for b in range(26)], dtype=np.uint64)[:, None]
        host = np.random.default_rng(logN).integers(0, 1 << 62, size=(26, N), dtype=np.uint64) % q
        for inverse in (False, True):
            outs = []
            for variant in (0, 1):
                d = ll.DeviceBuffer.from_host(host)
                ctx.ntt(d, 26, inverse=inverse, prime_base=0, prime_period=K, variant=variant)
                outs.append(d.to_host())
            assert (outs[0] == outs[1]).all(), (logN, inverse)
        big = ll.DeviceBuffer((max(counts), N))
        fill = (np.arange(max(counts) * N, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(5)
        L.dc_memcpy_h2d(big.ptr, fill.ctypes.data, fill.nbytes)
        for inverse in (False, True):
            for count in counts:
                iters = max(20, min(2000, (1 << 26) // (count * N)))
                t = np.array([[window(L, ctx, big, count, inverse, v, iters, ev) for v in (0, 1, 0)] for _ in range(a.rounds)]).mean(axis=0)
                base, gain, spread = (t[0] + t[2]) / 2, t[1] - (t[0] + t[2]) / 2, abs(t[0] - t[2])
                ok = gain < 0 and -gain > 5 * spread
                passes[(logN, inverse, count)] = ok
                lines.append(f"N=2^{logN} {'inv' if inverse else 'fwd'} limbs {count:5d} ({iters:4d} launches per window): two-launch A {t[0]:9.2f}  single "
                             f"{t[1]:9.2f}  two-launch B {t[2]:9.2f} us | per limb {base / count:7.3f} / {t[1] / count:7.3f} | 1 - 0 {gain:+9.2f} us "
                             f"({gain / base * 100:+6.1f} %)  0/0 spread {spread:6.2f} | {'clears the bar' if ok else 'does not'}")
                print(lines[-1], flush=True)
    lines.append("")
    for inverse in (False, True):  # one threshold per direction for all three rings: the smallest count from which every measured case passes
        counts = sorted({c for (_, inv, c) in passes if inv == inverse})
        good = [c for c in counts if all(ok for (_, inv, cc), ok in passes.items() if inv == inverse and cc >= c)]
        lines.append(f"{'ntt_lds_inv_min_limbs' if inverse else 'ntt_lds_min_limbs'}: " +
                     (f"every measured case from {good[0]} limbs on clears the bar" if good else "no threshold clears the bar on all three rings: 0 (never)"))
        print(lines[-1])
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
