#!/usr/bin/env python3
"""Do two builds of the library LAUNCH the same things?  (What a refactor of the launch rules -- csrc/launch_shape.hpp, kernels.hpp ntt_kind --
has to show.)
    python tools/legs/launch_identity.py PARENT_LIB BRANCH_LIB [--part traces|kernels] [--out profiles/launch_shape_refactor.txt]
Part "traces": plan_identity.py's comparison (option trace = 2, the plan's text on file descriptor 2 byte for byte, the VM's counters) of the
headline fixture and of the conv-shaped program under every option set below that moves a key switch or a transform to another launch sequence.
Part "kernels": a short program (N = 2^12, 4 primes: one rotation, one multiply and rescale, one sum of three rotations) under
`rocprofv3 --kernel-trace` (no counters), once per library and option set; the sequences of (kernel name, grid) in dispatch order must be equal.
Every run is a process of its own (DACAPO_AMD_LIB selects the build) under its own time limit (timeout -k 10 300)."""
import csv
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from plan_identity import conv_program, plan_text  # noqa: E402

OPTSETS = {
    "defaults": {},
    "ks_fuse_mac=0": {"ks_fuse_mac": 0},
    "ks_big_tiles=1": {"ks_big_tiles": 1},
    "ks_fuse_mac_tiles=72": {"ks_fuse_mac_tiles": 72},
    "ks_fold_add=0": {"ks_fold_add": 0},
    "ks_hoist=1 ks_lazy_sum=1": {"ks_hoist": 1, "ks_lazy_sum": 1},
    "ks_fold_rescale=1": {"ks_fold_rescale": 1},
    "ntt_lds_min_limbs=8 ntt_lds_inv_min_limbs=8": {"ntt_lds_min_limbs": 8, "ntt_lds_inv_min_limbs": 8},  # (N = 2^12 programs only)
}
LDS = "ntt_lds_min_limbs=8 ntt_lds_inv_min_limbs=8"
TRACE_RUNS = [(p, o) for p in ("headline", "conv13") for o in OPTSETS if o != LDS] + [("conv12", LDS)]


def short_program(slots):
    import numpy as np

    from dacapo_amd import hevm_asm as ha

    rng = np.random.default_rng(5)
    b = ha.Builder(slots=slots, init_level=3, policy="lazy", boot_level=3, shadow=True)
    x, y = b.input(rng.uniform(-1, 1, slots)), b.input(rng.uniform(-1, 1, slots))
    m = b.hint(b.mul(b.rotate(x, 1), y), 0)  # one rotation, one multiply and its rescale
    b.output(b.finish(b.add(b.add(b.rotate(m, 1), b.rotate(m, 2)), b.rotate(m, 4))))  # a hoisted lazy sum under ks_hoist, ks_lazy_sum
    return b


def child(program, optset):
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    opts = dict(OPTSETS[optset])
    if program == "headline":
        fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
        kw, cst, hv, inputs = dict(logN=15, num_primes=14), fx["cst"], fx["hevm"], [fx["packed"]]
    else:
        logN = int(program[-2:])
        if program.startswith("conv"):
            kw, b = dict(logN=logN, num_primes=6), conv_program(1 << (logN - 1), 5)
        else:  # one stream, no graph: the dispatch order is the plan's own
            kw, b = dict(logN=logN, num_primes=4), short_program(1 << (logN - 1))
            opts.update(plan_lanes=1, plan_graph=0)
        cst, hv, _ = b.assemble()
        inputs = [a.plain for a in b.args]
    if not program.startswith("short"):
        opts["trace"] = 2
    with runner.options(**opts):  # VM options are read at creation, launch shapes at every launch: both hold from here to the end of run()
        vm = runner.HEVM(fresh=True, **kw)
        vm.load_mem(cst, hv)
        for i, x in enumerate(inputs):
            vm.setInput(i, x)
        t0 = time.perf_counter()
        vm.run()
        ms = (time.perf_counter() - t0) * 1e3
        vm.getOutput()
    res = {"first_run_ms": ms, "stats": vm.stats(), "hoist": vm.hoist_stats(), "relin": vm.relin_stats(), "fold": vm.fold_rescale_stats()}
    vm.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_child(lib, program, optset, prefix=()):
    env = dict(os.environ, DACAPO_AMD_LIB=str(Path(lib).resolve()))
    env.pop("DACAPO_AMD_HOOKS", None)
    with tempfile.TemporaryFile(mode="w+b") as err:
        # (timeout(1) ends the whole tree at the limit: under a profiler the process that holds the GPU is a grandchild)
        p = subprocess.run(["timeout", "-k", "10", "300", *prefix, sys.executable, __file__, "--child", program, optset], env=env,
                           stdout=subprocess.PIPE, stderr=err)
        err.seek(0)
        text = err.read().decode(errors="replace")
    if p.returncode != 0:
        sys.stderr.write(text[-4000:])
        raise SystemExit(f"{program} under {optset} on {lib}: exit status {p.returncode}")
    return text, [json.loads(ln[7:]) for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")][0]


def kernel_sequence(lib, optset, tmp):
    """(kernel name, grid) of every dispatch of the short program, in dispatch order"""
    d = Path(tempfile.mkdtemp(dir=tmp))
    run_child(lib, "short12", optset, prefix=("rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", str(d), "--"))
    rows = []
    for f in sorted(d.rglob("*kernel_trace.csv")):
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"]) for r in rows]


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        return child(args[1], args[2])
    out, part = None, None
    for flag in ("--out", "--part"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                out = args[i + 1]
            else:
                part = args[i + 1]
            del args[i:i + 2]
    parent, branch = args
    lines, differ = [], 0

    def say(s):
        print(s, flush=True)
        lines.append(s + "\n")

    if part in (None, "traces"):
        for program, optset in TRACE_RUNS:
            (ta, ra), (tb, rb) = run_child(parent, program, optset), run_child(branch, program, optset)
            ta, tb = plan_text(ta), plan_text(tb)
            same, counters = ta == tb and len(ta) > 0, all(ra[k] == rb[k] for k in ("stats", "hoist", "relin", "fold"))
            differ += (not same) + (not counters)
            launches = [ln.split(" waves, ")[1].split(",")[0] for ln in tb.splitlines() if " pseudo-ops -> " in ln and " waves, " in ln]
            say(f"{program} {optset}: plan trace {len(ta.splitlines())} lines / {len(ta)} bytes on the parent, {len(tb.splitlines())} / {len(tb)} on the "
                f"branch: {'equal line for line' if same else 'DIFFERENT'}; counters {'equal' if counters else 'DIFFERENT'} (key switches "
                f"{rb['stats']['keyswitches']}, NTTs {rb['stats']['ntts']}, hops {rb['hoist']['hops']}, decompositions {rb['hoist']['decompositions']}, folded "
                f"pairs {rb['fold']}{', ' + launches[0] if launches else ''}); first run() {ra['first_run_ms']:.2f} / {rb['first_run_ms']:.2f} ms")
    if part in (None, "kernels"):
        with tempfile.TemporaryDirectory() as tmp:
            for optset in OPTSETS:
                ka, kb = kernel_sequence(parent, optset, tmp), kernel_sequence(branch, optset, tmp)
                same = ka == kb and len(ka) > 0
                differ += not same
                say(f"short12 {optset}: {len(ka)} dispatches on the parent, {len(kb)} on the branch, {len(set(k[0] for k in kb))} distinct kernels: "
                    f"(name, grid) sequence {'equal' if same else 'DIFFERENT'}")
                if not same:
                    for i, (a, b) in enumerate(zip(ka, kb)):
                        if a != b:
                            say(f"    first difference at dispatch {i}: {a} / {b}")
                            break
    say("every launch identical" if not differ else f"{differ} DIFFERENCES")
    if out:
        with open(out, "a") as fh:
            fh.write("".join(lines))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
