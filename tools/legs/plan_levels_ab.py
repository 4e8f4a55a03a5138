#!/usr/bin/env python3
"""A/B of the plan's levelling (option plan_level; csrc/plan_levels.cpp, csrc/plan_exec.hip sections 2 and 3b), one box, ONE process:
    python tools/legs/plan_levels_ab.py [--steps 7] [--out profiles/plan_levels_ab.txt] [--append FILE ...]
  (a) the headline plan as the trace option reports it, for plan_level 0 (ASAP), 1 (slack-aware levelling + addend hoist) and 2 (the hoist alone):
      steps by kind, waves, waves with more than one step, links, launches, live buffers, pool size; the VM's NTT and key-switch counts.
  (b) run(), wall clock around it (it returns after the stream has drained): the headline fixture on THREE VMs -- plan_level 0, 1, 0 -- whose runs
      alternate, --steps timed rounds each, mean (min .. max).  The two 0 VMs give the 0/0 spread: the gain counts only if it is larger than
      five times that spread.  rms against the committed torch logits: the limbs are identical for the same draws, so the rms values differ
      only by the fresh randomness of opcode 10.
  --lanes: instead of (b), plan_lanes 1 against 2 at plan_level 0 (the overlap the auxiliary stream gives the ASAP plan).
  --append: text files added verbatim (bench.py lines, kernel-trace summaries)."""
import os
import re
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s + "\n")


def fixture():
    from dacapo_amd import hevm_asm as ha

    return ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")


def rms_of(vm, fx):
    import numpy as np

    out = vm.getOutput()[0]
    return float(np.sqrt(np.mean((out[:10] * 32 - fx["torch_result"]) ** 2)))


class stderr_to_text:
    """the library writes its trace to file descriptor 2"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def make_vm(fx, opts, trace=False):
    from dacapo_amd import runner

    vm = runner.HEVM(fresh=True, logN=15, num_primes=14, vm_options=opts)
    text = ""
    if trace:
        with stderr_to_text() as cap, runner.options(trace=1):
            vm.load_mem(fx["cst"], fx["hevm"])
        text = cap.text
    else:
        vm.load_mem(fx["cst"], fx["hevm"])
    vm.setInput(0, fx["packed"])
    for _ in range(2):  # warm-up: the first run records the graph
        vm.run()
    return vm, text


def plan_leg(fx):
    for level in (0, 1, 2):
        vm, text = make_vm(fx, {"plan_level": level}, trace=True)
        kinds = re.findall(r"plan:\s+(\w+)\s+(\d+) steps\s+(\d+) items", text)
        say(f"plan_level {level}: steps by kind (steps/items) " + "  ".join(f"{k} {s}/{i}" for k, s, i in kinds))
        for line in text.splitlines():
            if "plan levels:" in line or " pseudo-ops -> " in line:
                say(f"plan_level {level}: " + line.replace("[dacapo_amd] ", ""))
        st = vm.stats()
        say(f"plan_level {level}: stats ntts {st['ntts']} keyswitches {st['keyswitches']}   rms vs torch logits {rms_of(vm, fx):.3e}")
        vm.close()


def timed(vms, steps):
    for _ in range(steps):
        for _, vm, ts in vms:
            t0 = time.perf_counter()
            vm.run()
            ts.append((time.perf_counter() - t0) * 1e3)
    mean = {}
    for name, vm, ts in vms:
        mean[name] = sum(ts) / len(ts)
        say(f"run headline {name:16s}: mean {mean[name]:8.2f} ms ({min(ts):.2f} .. {max(ts):.2f})")
    return mean


def ab_leg(fx, steps):
    vms = [(name, make_vm(fx, {"plan_level": level})[0], []) for name, level in (("plan_level 0 A", 0), ("plan_level 1", 1), ("plan_level 0 B", 0))]
    mean = timed(vms, steps)
    off, spread = 0.5 * (mean["plan_level 0 A"] + mean["plan_level 0 B"]), abs(mean["plan_level 0 A"] - mean["plan_level 0 B"])
    diff = mean["plan_level 1"] - off
    say(f"run headline 1 - 0 {diff:+7.2f} ms   0/0 spread {spread:6.2f} ms   "
        f"{'clears' if diff < 0 and -diff > 5 * spread else 'does NOT clear'} the bar (negative and larger than 5 x spread)")
    for _, vm, _ in vms:
        say(f"rms vs torch logits {rms_of(vm, fx):.3e}")
        vm.close()


def lanes_leg(fx, steps):
    vms = [(f"plan_lanes {lanes}", make_vm(fx, {"plan_lanes": lanes})[0], []) for lanes in (1, 2)]
    timed(vms, steps)
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

    steps, out = int(opt("--steps", 7)), opt("--out", None)
    extra = []
    if "--append" in args:
        i = args.index("--append")
        extra = args[i + 1:]
        del args[i:]
    fx = fixture()
    if "--lanes" in args:
        lanes_leg(fx, steps)
    elif "--plan-only" in args:
        plan_leg(fx)
    else:
        plan_leg(fx)
        ab_leg(fx, steps)
    for f in extra:
        LINES.append(Path(f).read_text())
    if out:
        with open(out, "a") as fh:
            fh.write("".join(LINES))


if __name__ == "__main__":
    main()
