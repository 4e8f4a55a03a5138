#!/usr/bin/env python3
"""A/B of option ks_fold_add (csrc/plan_exec.hip section 3a; csrc/fused_ks.hip f_ks_frows_mac_kernel), one box, ONE process:
    python tools/legs/ks_fold_add_ab.py [--steps 7] [--out profiles/ks_fold_add_ab.txt] [--append FILE ...]
  (a) the headline plan as the trace option reports it under ks_fold_add 0 and 1: steps by kind, waves, step launches, folds, live buffers;
      the VM's NTT and key-switch counts and the folds the run executed.
  (b) run(), wall clock around it: the headline fixture on THREE VMs -- ks_fold_add 0, 1, 0 -- whose runs alternate, --steps timed rounds each,
      mean (min .. max).  The two 0 VMs give the 0/0 spread: the gain counts only if it is negative and larger than five times that spread
      (the rule of profiles/plan_levels_ab.txt).  rms against the committed torch logits per VM.
  --plan-only: (a) alone.  --append: text files added verbatim (bench.py lines, kernel-trace summaries of tools/summarize/fold_add_trace.py,
  the compile-time register table)."""
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from plan_levels_ab import LINES, fixture, make_vm, rms_of, say, timed  # noqa: E402  (the same fixture, VM set-up and timing loop)


def plan_leg(fx):
    for on in (0, 1):
        vm, text = make_vm(fx, {"ks_fold_add": on}, trace=True)
        kinds = re.findall(r"plan:\s+(\w+)\s+(\d+) steps\s+(\d+) items", text)
        say(f"ks_fold_add {on}: steps by kind (steps/items) " + "  ".join(f"{k} {s}/{i}" for k, s, i in kinds))
        for line in text.splitlines():
            if "plan levels:" in line or " pseudo-ops -> " in line or "plan folds:" in line:
                say(f"ks_fold_add {on}: " + line.replace("[dacapo_amd] ", ""))
        st = vm.stats()
        say(f"ks_fold_add {on}: stats ntts {st['ntts']} keyswitches {st['keyswitches']} add_folds {st['add_folds']}   rms vs torch logits {rms_of(vm, fx):.3e}")
        vm.close()


def ab_leg(fx, steps):
    vms = [(name, make_vm(fx, {"ks_fold_add": on})[0], []) for name, on in (("ks_fold_add 0 A", 0), ("ks_fold_add 1", 1), ("ks_fold_add 0 B", 0))]
    mean = timed(vms, steps)
    off, spread = 0.5 * (mean["ks_fold_add 0 A"] + mean["ks_fold_add 0 B"]), abs(mean["ks_fold_add 0 A"] - mean["ks_fold_add 0 B"])
    diff = mean["ks_fold_add 1"] - off
    say(f"run headline 1 - 0 {diff:+7.2f} ms   0/0 spread {spread:6.2f} ms   "
        f"{'clears' if diff < 0 and -diff > 5 * spread else 'does NOT clear'} the bar (negative and larger than 5 x spread)")
    for name, vm, _ in vms:
        st = vm.stats()
        say(f"{name:16s}: ntts {st['ntts']} keyswitches {st['keyswitches']} add_folds {st['add_folds']}   rms vs torch logits {rms_of(vm, fx):.3e}")
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
    plan_leg(fx)
    if "--plan-only" not in args:
        ab_leg(fx, steps)
    for f in extra:
        LINES.append(Path(f).read_text())
    if out:
        with open(out, "a") as fh:
            fh.write("".join(LINES))


if __name__ == "__main__":
    main()
