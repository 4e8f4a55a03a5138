#!/usr/bin/env python3
"""A/B of lazy sums on SEAL-layout keys (option ks_lazy_sum with ks_hoist; csrc/hoist_ks.hip f_ks_gsum_kernel), one box, one process order:
    python tools/legs/ks_lazy_sum_ab.py [--steps 5] [--out profiles/ks_lazy_sum_ab.txt]
The headline fixture and its 13-prime lowering (resnet20.b13) under four settings -- the default options, ks_hoist = 1, ks_hoist = 1 with
ks_lazy_sum = 1, and with ks_lazy_sum = 2 -- wall clock around run() (it returns after the stream has drained; best of --steps): ms per run,
the plan's groups and their members (hevm_plan_lazy_groups), hops and decompositions, and rms against the committed torch logits.
Each setting is measured against the default run of the same session; differences below the box-to-box spread (profiles/README.md) are noise."""
import gzip
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

SETTINGS = [("default", {}), ("ks_hoist", {"ks_hoist": 1}), ("ks_hoist+lazy1", {"ks_hoist": 1, "ks_lazy_sum": 1}),
            ("ks_hoist+lazy2", {"ks_hoist": 1, "ks_lazy_sum": 2})]


def run_leg(tag, setting, steps):
    import numpy as np

    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    name, opts = SETTINGS[setting]
    fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
    hv = fx["hevm"] if tag == "headline" else gzip.open(ROOT / "tests" / "golden" / f"resnet20.{tag}.hevm.gz").read()
    vm = runner.HEVM(fresh=True, logN=15, num_primes=14, vm_options=opts)
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
    st, groups = vm.hoist_stats(), vm.lazy_groups()
    print(f"run {tag:8s} {name:15s}: {best * 1e3:8.2f} ms   groups {len(groups):3d}   members {sum(len(g) for g in groups):4d}   "
          f"hops {st['hops']:5d}   decompositions {st['decompositions']:5d}   rms vs torch logits {rms:.3e}", flush=True)
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

    steps, out = int(opt("--steps", 5)), opt("--out", None)
    if args and args[0] == "--child":
        run_leg(args[1], int(args[2]), steps)
        return
    lines = []
    for tag in ("headline", "b13"):
        for k in range(len(SETTINGS)):  # a fresh child per setting (VM options are read at creation; nothing of one setting is warm for the next)
            r = subprocess.run([sys.executable, __file__, "--steps", str(steps), "--child", tag, str(k)], capture_output=True, text=True, timeout=900)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"setting {tag} / {SETTINGS[k][0]} failed with status {r.returncode}")
            lines.append(r.stdout)
    if out:
        Path(out).write_text("".join(lines))


if __name__ == "__main__":
    main()
