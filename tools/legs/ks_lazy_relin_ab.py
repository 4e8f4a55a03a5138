#!/usr/bin/env python3
"""A/B of lazy relinearisation at the kernel-level ABI (dc_ct_mul_sum_relin; csrc/fused_ks.hip f_irows_tensor_sum_kernel /
f_frows_sum_final_kernel), one box, ONE process, warm-up first:
    python tools/legs/ks_lazy_relin_ab.py [--rounds 5] [--calls 50] [--steps 20] [--out profiles/ks_lazy_relin_ab.txt] [--skip-run]
  (a) per sum, device events: n x dc_ct_mul_relin + (n - 1) x dc_ct_add against ONE dc_ct_mul_sum_relin for n = 2, 3, 8 products at N = 2^15,
l = 2 and l = 13.  The two forms alternate, --rounds rounds of --calls sums each; mean and spread (min .. max) of the rounds, us per sum.
dc_ct_mul_sum_relin's time includes its synchronous copy of the term table (the call waits for the stream), so back-to-back calls do not
overlap host and device work as the separate form's do: the figure is the call as a host sees it.
  (b) run(), wall clock around it (it returns after the stream has drained): suite/Multivariate (three groups of three products, 6 key switches
      saved) on THREE VMs -- option ks_lazy_relin off, on, off again -- whose runs alternate, --steps timed rounds each.  The two off VMs give
      the off/off spread that the off/on difference has to be read against.  Groups, key switches and rms against the fixture's cleartext result.
The rounding differs (one mod-down instead of n), so the two results are not compared here: tests/test_gpu_lazy_relin.py pins both to the
oracle.  No speed-up is fixed in advance: where the lazy form loses, the line says so."""
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s + "\n")


def op_leg(logN, K, levels, counts, rounds, calls):
    import numpy as np

    from dacapo_amd import lowlevel as ll

    L, N = ll.lib(), 1 << logN
    ctx = ll.Context(logN, K)
    rng = np.random.default_rng(1)
    q = np.array(ctx.primes, dtype=np.uint64)
    key = rng.integers(0, 1 << 59, size=(K - 1, 2, K, N), dtype=np.uint64) % q[None, None, :, None]  # timing only: any residues
    dkey = ll.DeviceBuffer.from_host(key)
    del key
    e0, e1 = L.dc_event_create(), L.dc_event_create()
    for ell in levels:
        st = ell * N
        pool = [ll.DeviceBuffer.from_host(rng.integers(0, 1 << 59, size=(2, ell, N), dtype=np.uint64) % q[None, :ell, None]) for _ in range(2 * max(counts))]
        prods = [ll.DeviceBuffer((2, ell, N)) for _ in range(max(counts))]
        lazy = ll.DeviceBuffer((2, ell, N))
        for n in counts:
            a, b = [pool[2 * k].ptr for k in range(n)], [pool[2 * k + 1].ptr for k in range(n)]

            def separate():
                for k in range(n):
                    L.dc_ct_mul_relin(ctx.h, prods[k].ptr, st, a[k], st, b[k], st, dkey.ptr, ell, None)
                for k in range(1, n):
                    L.dc_ct_add(ctx.h, prods[0].ptr, st, prods[0].ptr, st, prods[k].ptr, st, ell, None)

            def summed():
                ctx.mul_sum_relin(lazy.ptr, st, a, b, [1] * n, st, dkey.ptr, ell)

            def timed(fn):
                L.dc_event_record(e0, None)
                for _ in range(calls):
                    fn()
                L.dc_event_record(e1, None)
                return L.dc_event_elapsed_ms(e0, e1) * 1e3 / calls

            for fn in (separate, summed):  # warm-up
                for _ in range(5):
                    fn()
            L.dc_stream_sync(None)
            t = {"separate": [], "summed": []}
            for _ in range(rounds):
                t["separate"].append(timed(separate))
                t["summed"].append(timed(summed))
            m = {k: sum(v) / len(v) for k, v in t.items()}
            verdict = "lazy form faster" if max(t["summed"]) < min(t["separate"]) else "lazy form SLOWER" if min(t["summed"]) > max(t["separate"]) else "within the spread"
            say(f"op N=2^{logN} l={ell:2d} n={n}: {n} x dc_ct_mul_relin + {n - 1} x dc_ct_add {m['separate']:8.1f} us ({min(t['separate']):.1f} .. {max(t['separate']):.1f})   "
                f"dc_ct_mul_sum_relin {m['summed']:8.1f} us ({min(t['summed']):.1f} .. {max(t['summed']):.1f})   "
                f"difference {m['summed'] - m['separate']:+8.1f} us   ratio {m['summed'] / m['separate']:5.3f}   {verdict}")


def run_leg(name, steps):
    import numpy as np

    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    fx = ha.read_fixture(ROOT / "tests" / "golden" / "suite" / name)
    vms = []
    for tag, lazy in (("off A", 0), ("on", 1), ("off B", 0)):
        vm = runner.HEVM(fresh=True, logN=15, num_primes=14, vm_options={"ks_lazy_relin": lazy})
        vm.load_mem(fx["cst"], fx["hevm"])
        for i, x in enumerate(fx["inputs"]):
            vm.setInput(i, x)
        for _ in range(3):  # warm-up
            vm.run()
        vms.append((tag, vm, []))
    for _ in range(steps):
        for _, vm, ts in vms:
            t0 = time.perf_counter()
            vm.run()
            ts.append((time.perf_counter() - t0) * 1e3)
    mean = {}
    for tag, vm, ts in vms:
        rms = float(np.sqrt(np.mean((vm.getOutput() - fx["expected"]) ** 2)))
        mean[tag] = sum(ts) / len(ts)
        rs = vm.relin_stats()
        say(f"run {name} ks_lazy_relin {tag:5s}: mean {mean[tag]:8.3f} ms ({min(ts):.3f} .. {max(ts):.3f})   groups {rs['groups']} products {rs['products']}   "
            f"key switches {vm.stats()['keyswitches']:3d}   rms vs cleartext {rms:.3e}")
    off = 0.5 * (mean["off A"] + mean["off B"])
    say(f"run {name} on - off {mean['on'] - off:+8.3f} ms   off/off spread {abs(mean['off A'] - mean['off B']):6.3f} ms")
    for _, vm, _ in vms:
        vm.close()


def main():
    args = sys.argv[1:]

    def opt(name, default):
        if name in args:
            i = args.index(name)
            v = args[i + 1]
            del args[i:i + 2]
            return v
        return default

    rounds, calls, steps, out = int(opt("--rounds", 5)), int(opt("--calls", 50)), int(opt("--steps", 20)), opt("--out", None)
    op_leg(15, 14, (2, 13), (2, 3, 8), rounds, calls)
    if "--skip-run" not in args:
        run_leg("Multivariate", steps)
    if out:
        Path(out).write_text("".join(LINES))


if __name__ == "__main__":
    main()
