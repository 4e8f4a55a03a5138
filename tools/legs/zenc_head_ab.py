#!/usr/bin/env python3
"""A/B of the zero-encryption head of run() (option zenc_head; csrc/hevm_vm.hip HEVM::plan_zero_encrypt), one box, ONE process, warm-up first:
    python tools/legs/zenc_head_ab.py [--steps 5] [--out profiles/zenc_head_ab.txt] [--append FILE ...]
    DACAPO_AMD_HOOKS=1 python tools/legs/zenc_head_ab.py --sweep [--steps 5] [--out FILE]
  (a) run(), wall clock around it (it returns after the stream has drained): the headline fixture on THREE VMs -- zenc_head = 0, 1, 0 -- whose
      runs alternate, --steps timed rounds each, mean (min .. max).  The two 0 VMs give the 0/0 spread that the 1-versus-0 difference has to be
      read against: the option defaults to 1 only if that difference is negative and larger than three times the spread.  rms against the
      committed torch logits: the limbs of both forms are identical for the same draws, so the rms values differ only by the fresh randomness.
  (b) --sweep (the hooks build: the chunk size is a constant of the release build, csrc/hevm_vm.hpp kZencChunk; HEVM_TEST_ZENC_CHUNK sizes
      it for seeded VMs): the same run() with zenc_head = 1 and 64 / 128 / 192 / 256 items per chunk, one VM each, runs alternating.
  --append: text files added verbatim (the head's own duration from a kernel trace, tools/summarize/zenc_head.py; bench.py lines).
No speed-up is fixed in advance: a difference within three times the 0/0 spread is recorded as no difference."""
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s + "\n")


def timed_rounds(vms, steps):
    for _ in range(steps):
        for _, vm, ts in vms:
            t0 = time.perf_counter()
            vm.run()
            ts.append((time.perf_counter() - t0) * 1e3)


def fixture():
    from dacapo_amd import hevm_asm as ha

    return ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")


def rms_of(vm, fx):
    import numpy as np

    out = vm.getOutput()[0]
    return float(np.sqrt(np.mean((out[:10] * 32 - fx["torch_result"]) ** 2)))


def ab_leg(steps):
    from dacapo_amd import runner

    fx = fixture()
    vms = []
    for name, head in (("0 A", 0), ("1", 1), ("0 B", 0)):
        vm = runner.HEVM(fresh=True, logN=15, num_primes=14, vm_options={"zenc_head": head})
        vm.load_mem(fx["cst"], fx["hevm"])
        vm.setInput(0, fx["packed"])
        for _ in range(2):  # warm-up: the first run records the graph
            vm.run()
        vms.append((name, vm, []))
    timed_rounds(vms, steps)
    mean = {}
    for name, vm, ts in vms:
        mean[name] = sum(ts) / len(ts)
        say(f"run headline zenc_head {name:3s}: mean {mean[name]:8.2f} ms ({min(ts):.2f} .. {max(ts):.2f})   "
            f"rms vs torch logits {rms_of(vm, fx):.3e}")
    off, spread = 0.5 * (mean["0 A"] + mean["0 B"]), abs(mean["0 A"] - mean["0 B"])
    diff = mean["1"] - off
    say(f"run headline 1 - 0 {diff:+7.2f} ms   0/0 spread {spread:6.2f} ms   "
        f"{'clears' if diff < 0 and -diff > 3 * spread else 'does NOT clear'} the bar (negative and larger than 3 x spread)")
    for _, vm, _ in vms:
        vm.close()


def sweep_leg(steps):
    from dacapo_amd import runner

    fx = fixture()
    vms = []
    for chunk in (64, 128, 192, 256):
        os.environ["HEVM_TEST_ZENC_CHUNK"] = str(chunk)
        vm = runner.HEVM(seed=0x4845564D, logN=15, num_primes=14, vm_options={"zenc_head": 1})
        del os.environ["HEVM_TEST_ZENC_CHUNK"]
        vm.load_mem(fx["cst"], fx["hevm"])
        vm.setInput(0, fx["packed"])
        for _ in range(2):
            vm.run()
        vms.append((chunk, vm, []))
    timed_rounds(vms, steps)
    for chunk, vm, ts in vms:
        say(f"run headline zenc_head 1, {chunk:3d} items per chunk (hooks build): mean {sum(ts) / len(ts):8.2f} ms ({min(ts):.2f} .. {max(ts):.2f})   "
            f"rms vs torch logits {rms_of(vm, fx):.3e}")
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

    steps, out = int(opt("--steps", 5)), opt("--out", None)
    extra = []
    if "--append" in args:
        i = args.index("--append")
        extra = args[i + 1:]
        del args[i:]
    if "--sweep" in args:
        sweep_leg(steps)
    else:
        ab_leg(steps)
    for f in extra:
        LINES.append(Path(f).read_text())
    if out:
        with open(out, "a") as fh:
            fh.write("".join(LINES))


if __name__ == "__main__":
    main()
