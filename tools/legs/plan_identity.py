#!/usr/bin/env python3
"""Do two builds of the library build the SAME plans?  (What a refactor of csrc/plan_exec.hip's builder has to show.)
    python tools/legs/plan_identity.py PARENT_LIB BRANCH_LIB [--out profiles/plan_builder_identity.txt] [--skip-headline]
Every case runs once per library in a process of its own (DACAPO_AMD_LIB selects the build) with option trace = 2: the library writes the plan
it builds to file descriptor 2 -- the first 400 steps wave by wave with kind, level, item count and lane, steps and items by kind and by
(kind, level), the sums that share sources, the producer -> consumer edges, links, launches, live and pool buffers.  The two texts must be
byte-identical.  Cases: the headline ResNet-20 fixture at default options, and a convolution-shaped program (tests/gpu_helpers.py
run_conv_shaped_program's shape) at N = 2^13 under one option set each.  Each child also reports the VM's counters after run(), the wall time
of load (constants, plaintext encoding, plan and graph: preprocess()) and of the first run(), and -- the conv-shaped cases -- the largest
error against the cleartext evaluation."""
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

# name -> (HEVM keyword arguments, streams)
CASES = {
    "headline default": (dict(logN=15, num_primes=14), 1),
    "conv plan_level=0": (dict(vm_options={"plan_level": 0}), 1),
    "conv chain_fusion=0": (dict(vm_options={"chain_fusion": 0}), 1),
    "conv plan_lanes=1": (dict(vm_options={"plan_lanes": 1}), 1),
    "conv online_encode=1": (dict(vm_options={"online_encode": 1}), 1),
    "conv rot_compose=1": (dict(vm_options={"rot_compose": 1}), 1),
    "conv ks_hoist=1 ks_lazy_sum=2": (dict(vm_options={"ks_hoist": 1, "ks_lazy_sum": 2}), 1),
    "conv ks_fold_rescale=1": (dict(vm_options={"ks_fold_rescale": 1}), 1),
    "conv ks_lazy_relin=1": (dict(vm_options={"ks_lazy_relin": 1}), 1),
    "conv 2 streams": (dict(), 2),
    "conv grouped digits hyb_lazy_sum=1 hyb_double_hoist=1": (dict(num_primes=8, ks_special=2, vm_options={"hyb_lazy_sum": 1, "hyb_double_hoist": 1}), 1),
}


def conv_program(slots, level):
    """19 rotated ct x pt products + 9 bare rotated ciphertexts summed, a second reader that is a rotation, then a square, a sum of two
    ct x ct products and the product of the two, each behind its rescale"""
    import numpy as np

    from dacapo_amd import hevm_asm as ha

    rng = np.random.default_rng(9)
    b = ha.Builder(slots=slots, init_level=level, policy="lazy", boot_level=level, shadow=True)
    x, y = b.input(rng.uniform(-1, 1, slots)), b.input(rng.uniform(-1, 1, slots))
    acc = None
    for k in range(19):
        t = b.mul_plain(b.rotate(x if k % 3 else y, 1 << (k % 7)), rng.uniform(-1, 1, slots))
        acc = t if acc is None else b.add(acc, t)
    z = b.mul_plain(y, rng.uniform(-1, 1, slots))
    for k in range(9):
        acc = b.add(acc, b.rotate(z, 3 + 2 * k))
    u = b.add(acc, b.rotate(acc, 5))
    sq = b.hint(b.mul(u, u), 0)                                   # a square and its rescale: a link, a merged step under ks_fold_rescale
    w = b.rotate(u, 2)
    pr = b.hint(b.add(b.mul(u, w), b.mul(w, w)), 0)                # a sum of two products at one level: a group under ks_lazy_relin
    b.output(b.finish(b.mul(sq, pr)))                              # a multiply behind two rescales: a CONT_MUL link
    return b


def child(name):
    import numpy as np

    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    kw, streams = CASES[name]
    kw = dict(kw)
    if name.startswith("headline"):
        fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
        cst, hv, inputs, expected = fx["cst"], fx["hevm"], [fx["packed"]], None
    else:
        kw.setdefault("num_primes", 6)
        kw["logN"] = 13
        b = conv_program(1 << 12, kw["num_primes"] - kw.get("ks_special", 1))
        cst, hv, _ = b.assemble()
        inputs, expected = [a.plain for a in b.args], b.expected()[0]
    vm = runner.HEVM(fresh=True, **kw)
    if streams > 1:
        vm.set_streams(streams)
    with runner.options(trace=2):
        t0 = time.perf_counter()
        vm.load_mem(cst, hv)
        t1 = time.perf_counter()
        for q in range(streams):
            vm.select_stream(q)
            for i, x in enumerate(inputs):
                vm.setInput(i, x)
        vm.select_stream(0)
        t2 = time.perf_counter()
        vm.run()
        t3 = time.perf_counter()
    out = vm.getOutput()[0]
    res = {"load_ms": (t1 - t0) * 1e3, "first_run_ms": (t3 - t2) * 1e3, "stats": vm.stats(), "hoist": vm.hoist_stats(), "relin": vm.relin_stats(),
           "fold": vm.fold_rescale_stats(), "max_error": None if expected is None else float(np.abs(out - expected).max())}
    vm.close()
    print("RESULT " + json.dumps(res), flush=True)


def plan_text(stderr_text):
    """the plan's trace: every "[dacapo_amd] plan..." line and the wave-by-wave listing"""
    return "".join(ln + "\n" for ln in stderr_text.splitlines() if ln.startswith("[dacapo_amd] plan") or ln.startswith("  wave "))


def run_case(lib, name):
    env = dict(os.environ, DACAPO_AMD_LIB=str(Path(lib).resolve()))
    env.pop("DACAPO_AMD_HOOKS", None)
    with tempfile.TemporaryFile(mode="w+b") as err:
        p = subprocess.run([sys.executable, __file__, "--child", name], env=env, stdout=subprocess.PIPE, stderr=err, timeout=600)
        err.seek(0)
        text = err.read().decode(errors="replace")
    if p.returncode != 0:
        sys.stderr.write(text[-4000:])
        raise SystemExit(f"{name} on {lib}: exit status {p.returncode}")
    res = [json.loads(ln[7:]) for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")][0]
    return plan_text(text), res


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        return child(args[1])
    out = None
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    skip_headline = "--skip-headline" in args
    args = [a for a in args if a != "--skip-headline"]
    parent, branch = args
    lines, differ = [], 0

    def say(s):
        print(s, flush=True)
        lines.append(s + "\n")

    for name in CASES:
        if skip_headline and name.startswith("headline"):
            continue
        (ta, ra), (tb, rb) = run_case(parent, name), run_case(branch, name)
        same = ta == tb and len(ta) > 0
        counters = all(ra[k] == rb[k] for k in ("stats", "hoist", "relin", "fold"))
        differ += (not same) + (not counters)
        summary = [ln for ln in tb.splitlines() if " pseudo-ops -> " in ln]
        say(f"{name}: plan trace {len(ta.splitlines())} lines / {len(ta)} bytes on the parent, {len(tb.splitlines())} / {len(tb)} on the branch: "
            f"{'byte-identical' if same else 'DIFFERENT'}; counters {'equal' if counters else 'DIFFERENT'} "
            f"(key switches {rb['stats']['keyswitches']}, NTTs {rb['stats']['ntts']}, hops {rb['hoist']['hops']}, decompositions {rb['hoist']['decompositions']}, "
            f"relin groups {rb['relin']['groups']}, folded pairs {rb['fold']})")
        if summary:
            say("    " + summary[0].replace("[dacapo_amd] ", ""))
        say(f"    load (preprocess: encode, plan, graph) {ra['load_ms']:.1f} ms parent / {rb['load_ms']:.1f} ms branch; first run() {ra['first_run_ms']:.2f} / {rb['first_run_ms']:.2f} ms"
            + ("" if rb["max_error"] is None else f"; largest error against the cleartext {ra['max_error']:.2e} / {rb['max_error']:.2e}"))
        if not same:
            import difflib

            for ln in list(difflib.unified_diff(ta.splitlines(), tb.splitlines(), "parent", "branch", lineterm="", n=0))[:20]:
                say("    " + ln)
    say(f"{'every plan identical' if not differ else str(differ) + ' DIFFERENCES'}")
    if out:
        with open(out, "a") as fh:
            fh.write("".join(lines))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
