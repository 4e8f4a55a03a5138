#!/usr/bin/env python3
"""A/B of flattened rotate-and-add chains (option ks_flatten_sums; csrc/plan_flatten.cpp, hoist_ks.hip f_ks_gsum_kernel with an addend), one box,
one process:
    python tools/legs/ks_flatten_ab.py [--steps 10] [--fs 2,3,4,6] [--streams 1,8] [--out profiles/ks_flatten_ab.txt] [--tag TEXT]
  * run() of the headline program (tests/golden/resnet20) per stream count on VMs whose runs alternate, --steps timed rounds after 3 warm-up
    runs: option ks_flatten_sums off (A), then per f a VM with it on, and off again (B).  ks_hoist = 1 and ks_lazy_sum = 2 in every arm, so that
    only the flattening differs; the two off VMs give the spread that every difference is read against.  One default-options VM beside them
    for scale.  Per VM: the plan's own report (option trace: pseudo-ops, steps, waves, launches), key switches, the flattened groups, the
    composite keys added and the HBM they take, the rms against the torch logits.
  * --only-default: just the default-options VM (what a run on another build of the library, DACAPO_AMD_LIB, is compared by).
  * --trace-f F: ONE VM with ks_flatten_sums = F (0: off) and three run()s, nothing else -- the process to put under a kernel trace."""
import os
import re
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def captured_stderr(fn):
    """fn() with the process's stderr (the library writes its plan report there) going to a file -> the text"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode("utf-8", "replace")


def make_vm(fx, opts, streams):
    """a fresh-key VM with the program loaded, the composite keys added, inputs set, the plan built under option trace and 3 warm-up runs
    -> (vm, description)"""
    import numpy as np

    from dacapo_amd import runner

    vm = runner.HEVM(fresh=True, logN=15, num_primes=14, vm_options=opts)
    if streams > 1:
        vm.set_streams(streams)
    runner.set_option("trace", 1)  # (the plan is built when the program is loaded, and again after keys were added)
    report = captured_stderr(lambda: vm.load_mem(fx["cst"], fx["hevm"]))
    missing = vm.flatten_offsets() if opts.get("ks_flatten_sums") else []
    if missing:
        vm.addRotationKeys(missing)
    for q in range(streams):
        if streams > 1:
            vm.select_stream(q)
        vm.setInput(0, fx["packed"])
    report += captured_stderr(vm.run)
    runner.set_option("trace", 0)
    for _ in range(2):
        vm.run()
    found = re.findall(r"plan: (\d+) ops -> (\d+) pseudo-ops -> (\d+) steps .* in (\d+) waves, ~(\d+) launches", report)
    m = found[-1] if found else None
    plan = f"pseudo-ops {m[1]} steps {m[2]} waves {m[3]} launches ~{m[4]}" if m else "no plan report"
    if streams > 1:
        vm.select_stream(0)
    logits = vm.getOutput()[0][:10] * 32
    rms = float(np.sqrt(np.mean((logits - fx["torch_result"]) ** 2)))
    st = vm.stats()
    fs = vm.flatten_stats()
    key_mb = len(missing) * 13 * 2 * 14 * (1 << 15) * 8 / 2**20  # a Galois key: [digits][2][K][N] words
    desc = (f"{plan}   key switches {st['keyswitches']}  NTTs {st['ntts']}   groups {fs['groups']} members {fs['members']} hops absorbed {fs['hops_absorbed']}   "
            f"composite keys added {len(missing)} ({key_mb:.0f} MiB)   rms vs torch {rms:.3e}")
    return vm, desc


def timed_rounds(vms, steps):
    ts = [[] for _ in vms]
    for _ in range(steps):
        for k, vm in enumerate(vms):
            t0 = time.perf_counter()
            vm.run()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return ts


def fmt(ts):
    return f"mean {sum(ts) / len(ts):9.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def main():
    args = sys.argv[1:]

    def opt(name, default):
        if name in args:
            i = args.index(name)
            v = args[i + 1]
            del args[i:i + 2]
            return v
        return default

    steps, out, tag = int(opt("--steps", 10)), opt("--out", None), opt("--tag", "")
    fs = [int(x) for x in opt("--fs", "2,3,4,6").split(",")]
    stream_counts = [int(x) for x in opt("--streams", "1,8").split(",")]
    trace_f = opt("--trace-f", None)
    from dacapo_amd import hevm_asm as ha

    fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
    base = {"ks_hoist": 1, "ks_lazy_sum": 2}
    if trace_f is not None:
        f = int(trace_f)
        vm, desc = make_vm(fx, dict(base, ks_flatten_sums=f) if f else dict(base), 1)
        say(f"trace run ks_flatten_sums {f}: {desc}")
        vm.close()
        return
    if tag:
        say(f"# {tag}")
    if "--only-default" in args:
        for S in stream_counts:
            vm, desc = make_vm(fx, {}, S)
            ts = timed_rounds([vm], steps)[0]
            say(f"run resnet20 streams {S} default options       : {fmt(ts)}   {desc}")
            vm.close()
    else:
        for S in stream_counts:
            vm, desc = make_vm(fx, {}, S)
            say(f"run resnet20 streams {S} default options       : {fmt(timed_rounds([vm], steps)[0])}   {desc}")
            vm.close()
            off_a, desc_a = make_vm(fx, dict(base), S)
            off_b, desc_b = make_vm(fx, dict(base), S)
            say(f"run resnet20 streams {S} flatten off (plan)    : {desc_a}")
            for f in fs:
                on, desc = make_vm(fx, dict(base, ks_flatten_sums=f), S)
                ta, tn, tb = timed_rounds([off_a, on, off_b], steps)
                ma, mn, mb = (sum(t) / len(t) for t in (ta, tn, tb))
                say(f"run resnet20 streams {S} f = {f} off A          : {fmt(ta)}")
                say(f"run resnet20 streams {S} f = {f} on             : {fmt(tn)}   {desc}")
                say(f"run resnet20 streams {S} f = {f} off B          : {fmt(tb)}")
                say(f"run resnet20 streams {S} f = {f} on - off {mn - 0.5 * (ma + mb):+9.3f} ms ({100 * (mn / (0.5 * (ma + mb)) - 1):+.2f} %)   off/off spread {abs(ma - mb):7.3f} ms")
                on.close()
            off_a.close()
            off_b.close()
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        with open(out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
