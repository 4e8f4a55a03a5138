#!/usr/bin/env python3
"""A/B of hoisted rotations on SEAL-layout keys (option ks_hoist, dc_ct_rotate_hoisted; csrc/hoist_ks.hip), one box, one process per setting:
    python tools/legs/ks_hoist_ab.py [--reps 20] [--steps 5] [--out profiles/ks_hoist_ab.txt] [--skip-cfg3]
  (a) kernel level, device events: r = 1, 2, 4, 8 hops of ONE source as r calls of dc_ct_rotate_hop against one dc_ct_rotate_hoisted, at
      N = 2^15 / l = 13 and N = 2^16 / l = 24 (config 3's hop).  r = 1 shows what the stored decomposition costs when nothing shares it.
  (b) VM level, wall clock around run() (it returns after the stream has drained; best of --steps): the headline fixture and its 13-prime
      lowering with ks_hoist 0 and 1 -- hops, decompositions (hevm_last_run_hoist_stats) and rms against the committed torch logits.
The comparison is the option off against on in the same session; differences below the box-to-box spread (profiles/README.md) are noise."""
import ctypes as C
import gzip
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def kernel_leg(logN, K, ell, reps):
    import numpy as np

    from dacapo_amd import lowlevel as ll

    L, N = ll.lib(), 1 << logN
    ctx = ll.Context(logN, K)
    rng = np.random.default_rng(1)
    q = np.array(ctx.primes, dtype=np.uint64)
    key = rng.integers(0, 1 << 59, size=(K - 1, 2, K, N), dtype=np.uint64) % q[None, None, :, None]  # timing only: any residues
    src = rng.integers(0, 1 << 59, size=(2, ell, N), dtype=np.uint64) % q[None, :ell, None]
    R = 8
    dkeys = [ll.DeviceBuffer.from_host(key) for _ in range(R)]  # one buffer per hop: no two hops read the same key lines
    dsrc = ll.DeviceBuffer.from_host(src)
    outs = [ll.DeviceBuffer((2, ell, N)) for _ in range(R)]
    elts = [ctx.elt_from_step(s) for s in (1, 2, 3, 5, -1, 4, 8, -3)]
    st = ell * N
    e0, e1 = L.dc_event_create(), L.dc_event_create()

    def timed(fn):
        fn()
        L.dc_stream_sync(None)
        best = 1e9
        for _ in range(reps):
            L.dc_event_record(e0, None)
            fn()
            L.dc_event_record(e1, None)
            best = min(best, L.dc_event_elapsed_ms(e0, e1))
        return best * 1e3

    for r in (1, 2, 4, 8):
        def plain():
            for b in range(r):
                L.dc_ct_rotate_hop(ctx.h, outs[b].ptr, st, dsrc.ptr, st, elts[b], dkeys[b].ptr, ell, None)

        dsts = (C.c_void_p * r)(*[o.ptr for o in outs[:r]])
        keys = (C.c_void_p * r)(*[k.ptr for k in dkeys[:r]])
        ge = (C.c_uint32 * r)(*elts[:r])

        def hoisted():
            L.dc_ct_rotate_hoisted(ctx.h, dsts, st, dsrc.ptr, st, ge, keys, r, ell, None)

        a, b = timed(plain), timed(hoisted)
        print(f"kernel N=2^{logN} l={ell:2d} r={r}: {r} x dc_ct_rotate_hop {a:9.1f} us   dc_ct_rotate_hoisted {b:9.1f} us   ratio {b / a:5.3f}   "
              f"per hop {a / r:7.1f} -> {b / r:7.1f} us", flush=True)


def run_leg(tag, hoist, steps):
    import numpy as np

    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
    hv = fx["hevm"] if tag == "headline" else gzip.open(ROOT / "tests" / "golden" / f"resnet20.{tag}.hevm.gz").read()
    vm = runner.HEVM(fresh=True, logN=15, num_primes=14, vm_options={"ks_hoist": hoist})
    vm.load_mem(fx["cst"], hv)
    vm.setInput(0, fx["packed"])
    vm.run()
    best = 1e9
    for _ in range(steps):
        t0 = time.perf_counter()
        vm.run()
        best = min(best, time.perf_counter() - t0)
    out = vm.getOutput()[0]
    rms = float(np.sqrt(np.mean((out[:10] * 32 - fx["torch_result"]) ** 2)))
    st = vm.hoist_stats()
    print(f"run {tag:8s} ks_hoist={hoist}: {best * 1e3:8.2f} ms   hops {st['hops']:5d}   decompositions {st['decompositions']:5d}   "
          f"rms vs torch logits {rms:.3e}", flush=True)
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

    reps, steps, out = int(opt("--reps", 20)), int(opt("--steps", 5)), opt("--out", None)
    if args and args[0] == "--child":
        if args[1] == "kernel":
            kernel_leg(int(args[2]), int(args[3]), int(args[4]), reps)
        else:
            run_leg(args[2], int(args[3]), steps)
        return
    jobs = [["kernel", "15", "14", "13"]]
    if "--skip-cfg3" not in args:
        jobs.append(["kernel", "16", "25", "24"])
    jobs += [["run", tag, str(h)] for tag in ("headline", "b13") for h in (0, 1)]
    lines = []
    for j in jobs:  # a fresh child per setting (VM options are read at creation; nothing of one setting is warm for the next)
        r = subprocess.run([sys.executable, __file__, "--reps", str(reps), "--steps", str(steps), "--child"] + j, capture_output=True, text=True,
                           timeout=900)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"setting {j} failed with status {r.returncode}")
        lines.append(r.stdout)
    if out:
        Path(out).write_text("".join(lines))


if __name__ == "__main__":
    main()
