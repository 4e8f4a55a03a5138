#!/usr/bin/env python3
"""A/B of a rescale folded into the multiply's key switch (option ks_fold_rescale, dc_ct_mul_relin_rescale; csrc/fused_ks.hip
f_dr2_icols_lift_fcols_kernel), one box, ONE process, warm-up first:
    python tools/legs/ks_fold_rescale_ab.py [--rounds 5] [--calls 50] [--steps 5] [--out profiles/ks_fold_rescale_ab.txt] [--skip-cfg3] [--skip-run]
  (a) per op, device events: dc_ct_mul_relin followed by dc_ct_rescale against one dc_ct_mul_relin_rescale at N = 2^15, l = 2, 3, 5, 13 and at
      N = 2^16, l = 24.  The two forms alternate, --rounds rounds of --calls calls each; mean and spread (min .. max) of the rounds, us per call.
  (b) run(), wall clock around it (it returns after the stream has drained): the headline fixture and resnet20.b13 on THREE VMs -- option off,
      option on, option off again -- whose runs alternate, --steps timed rounds each.  The two off VMs give the off/off spread that the off/on
      difference has to be read against.  Pair count (hevm_last_run_fold_rescale_stats) and rms against the committed torch logits: the limbs
      are identical, so the rms values differ only by the fresh randomness of opcode 10.
No speed-up is fixed in advance: a difference within the off/off spread is recorded as no difference."""
import gzip
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s + "\n")


def op_leg(logN, K, levels, rounds, calls):
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
        a, b = (ll.DeviceBuffer.from_host(rng.integers(0, 1 << 59, size=(2, ell, N), dtype=np.uint64) % q[None, :ell, None]) for _ in range(2))
        prod, two, one = ll.DeviceBuffer((2, ell, N)), ll.DeviceBuffer((2, ell - 1, N)), ll.DeviceBuffer((2, ell - 1, N))
        st, st1 = ell * N, (ell - 1) * N

        def separate():
            L.dc_ct_mul_relin(ctx.h, prod.ptr, st, a.ptr, st, b.ptr, st, dkey.ptr, ell, None)
            L.dc_ct_rescale(ctx.h, two.ptr, st1, prod.ptr, st, ell, None)

        def folded():
            L.dc_ct_mul_relin_rescale(ctx.h, one.ptr, st1, a.ptr, st, b.ptr, st, dkey.ptr, None, None, ell, None)

        def timed(fn):
            L.dc_event_record(e0, None)
            for _ in range(calls):
                fn()
            L.dc_event_record(e1, None)
            return L.dc_event_elapsed_ms(e0, e1) * 1e3 / calls

        for fn in (separate, folded):  # warm-up
            for _ in range(5):
                fn()
        L.dc_stream_sync(None)
        assert (one.to_host() == two.to_host()).all()
        t = {"separate": [], "folded": []}
        for _ in range(rounds):
            t["separate"].append(timed(separate))
            t["folded"].append(timed(folded))
        m = {k: sum(v) / len(v) for k, v in t.items()}
        say(f"op N=2^{logN} l={ell:2d}: dc_ct_mul_relin + dc_ct_rescale {m['separate']:8.1f} us ({min(t['separate']):.1f} .. {max(t['separate']):.1f})   "
            f"dc_ct_mul_relin_rescale {m['folded']:8.1f} us ({min(t['folded']):.1f} .. {max(t['folded']):.1f})   "
            f"difference {m['folded'] - m['separate']:+7.1f} us   ratio {m['folded'] / m['separate']:5.3f}")


def run_leg(tag, steps):
    import numpy as np

    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
    hv = fx["hevm"] if tag == "headline" else gzip.open(ROOT / "tests" / "golden" / f"resnet20.{tag}.hevm.gz").read()
    vms = []
    for name, fold in (("off A", 0), ("on", 1), ("off B", 0)):
        vm = runner.HEVM(fresh=True, logN=15, num_primes=14, vm_options={"ks_fold_rescale": fold})
        vm.load_mem(fx["cst"], hv)
        vm.setInput(0, fx["packed"])
        vm.run()  # warm-up
        vms.append((name, vm, []))
    for _ in range(steps):
        for _, vm, ts in vms:
            t0 = time.perf_counter()
            vm.run()
            ts.append((time.perf_counter() - t0) * 1e3)
    mean = {}
    for name, vm, ts in vms:
        out = vm.getOutput()[0]
        rms = float(np.sqrt(np.mean((out[:10] * 32 - fx["torch_result"]) ** 2)))
        mean[name] = sum(ts) / len(ts)
        say(f"run {tag:8s} ks_fold_rescale {name:5s}: mean {mean[name]:8.2f} ms ({min(ts):.2f} .. {max(ts):.2f})   pairs {vm.fold_rescale_stats():4d}   "
            f"rms vs torch logits {rms:.3e}")
    off = 0.5 * (mean["off A"] + mean["off B"])
    say(f"run {tag:8s} on - off {mean['on'] - off:+7.2f} ms   off/off spread {abs(mean['off A'] - mean['off B']):6.2f} ms")
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

    rounds, calls, steps, out = int(opt("--rounds", 5)), int(opt("--calls", 50)), int(opt("--steps", 5)), opt("--out", None)
    op_leg(15, 14, (2, 3, 5, 13), rounds, calls)
    if "--skip-cfg3" not in args:
        op_leg(16, 25, (24,), rounds, calls)
    if "--skip-run" not in args:
        for tag in ("headline", "b13"):
            run_leg(tag, steps)
    if out:
        Path(out).write_text("".join(LINES))


if __name__ == "__main__":
    main()
