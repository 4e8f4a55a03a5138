#!/usr/bin/env python3
"""Batched against sequential input / output of the fed regime (hevm_encrypt_batch / hevm_decrypt_result_batch; csrc/hevm_vm.hip
HEVM::encrypt_batch / decrypt_batch), one box, ONE process, warm-up first:
    python tools/legs/io_batch_ab.py [--steps 10] [--streams 8] [--out profiles/io_batch_ab.txt]
One fresh VM at the reference's parameters (N = 2^15, 14 primes) with the headline fixture loaded and 8 streams.  Wall clock around
  inputs:   8 x (select_stream + setInput)   |   one setInputs from host memory   |   one setInputs from a torch tensor in HBM
  outputs:  8 x (select_stream + getOutput)  |   one getOutputs to host memory    |   one getOutputs into a torch tensor in HBM
the three forms of a direction alternating, --steps timed rounds each, mean (min .. max), with hevm_last_io_stats of the batch calls.  The
sequential calls are the parent commit's code, unchanged.  No speed-up is fixed in advance: what is measured is what is written.
(torch is imported BEFORE the library: it ships a HIP runtime of its own, and a process runs on the one that was loaded first.)"""
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s + "\n")


def rounds(forms, steps):
    """forms: [(name, callable)]; every form once per round, after one warm-up call each"""
    ts = {name: [] for name, _ in forms}
    for name, f in forms:
        f()
    for _ in range(steps):
        for name, f in forms:
            t0 = time.perf_counter()
            f()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    args = sys.argv[1:]

    def opt(name, default):
        if name in args:
            i = args.index(name)
            v = args[i + 1]
            del args[i:i + 2]
            return v
        return default

    steps, streams, out = int(opt("--steps", 10)), int(opt("--streams", 8)), opt("--out", None)
    try:
        import torch

        if not torch.cuda.is_available():
            torch = None
    except ImportError:
        torch = None
    import numpy as np

    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
    vm = runner.HEVM(fresh=True, logN=15, num_primes=14)
    vm.set_streams(streams)
    vm.load_mem(fx["cst"], fx["hevm"])
    packed = np.ascontiguousarray(fx["packed"], dtype=np.float64)
    data = np.stack([packed] * streams)
    say(f"io_batch_ab: N = 2^15, 14 primes, headline fixture, {streams} streams, input of {packed.size} doubles per stream, "
        f"{vm.reslen} result(s) of {vm.slots} doubles per stream; {steps} timed rounds after one warm-up call per form")

    def seq_in():
        for s in range(streams):
            vm.select_stream(s)
            vm.setInput(0, packed)
        vm.select_stream(0)

    stats = {}

    def host_in():
        vm.setInputs(0, data)
        stats["setInputs host"] = vm.io_stats()

    forms = [(f"{streams} x (select_stream + setInput)", seq_in), ("one setInputs, host", host_in)]
    if torch is not None:
        t_in = torch.tensor(data, dtype=torch.float64, device="cuda")

        def dev_in():
            vm.setInputs(0, t_in)
            stats["setInputs device"] = vm.io_stats()

        forms.append(("one setInputs, device", dev_in))
    else:
        say("inputs  one setInputs, device: NOT measured (torch sees no GPU in this process)")
    ts_in = rounds(forms, steps)
    import ctypes

    back = np.zeros((streams, vm.slots))  # what the last batch encrypted, decrypted again
    vm.lw.hevm_decrypt_batch(vm.vm, 0, back.ctypes.data_as(ctypes.c_void_p), vm.slots, 0, streams, 0)
    say(f"setInputs round trip (hevm_decrypt_batch of the input registers): max |decrypted - input| {np.abs(back - np.resize(packed, vm.slots)).max():.3e}")

    vm.run()  # the results the output forms read

    def seq_out():
        for s in range(streams):
            vm.select_stream(s)
            vm.getOutput()
        vm.select_stream(0)

    def host_out():
        vm.getOutputs()
        stats["getOutputs host"] = vm.io_stats()

    forms_out = [(f"{streams} x (select_stream + getOutput)", seq_out), ("one getOutputs, host", host_out)]
    if torch is not None:
        t_out = torch.zeros((streams, vm.reslen, vm.slots), dtype=torch.float64, device="cuda")

        def dev_out():
            vm.getOutputs(out=t_out)
            stats["getOutputs device"] = vm.io_stats()

        forms_out.append(("one getOutputs, device", dev_out))
    else:
        say("outputs one getOutputs, device: NOT measured (torch sees no GPU in this process)")
    ts_out = rounds(forms_out, steps)

    for label, ts in (("inputs ", ts_in), ("outputs", ts_out)):
        names = list(ts)
        base = sum(ts[names[0]]) / len(ts[names[0]])
        for name in names:
            t = ts[name]
            mean = sum(t) / len(t)
            rel = "" if name == names[0] else f"   {base / mean:5.2f} x the sequential calls' rate ({'faster' if mean < base else 'NOT faster'})"
            say(f"{label} {name:34s}: mean {mean:8.3f} ms ({min(t):.3f} .. {max(t):.3f}){rel}")
    for name, st in stats.items():
        say(f"hevm_last_io_stats after {name}: {st['launches']} launches in {st['chunks']} chunk(s)"
            + (" (per result)" if name.startswith("getOutputs") else ""))
    if torch is not None:  # the three output forms agree bit for bit
        a, b = vm.getOutputs(), t_out.cpu().numpy()
        say(f"getOutputs host == device bit for bit: {bool((a.view(np.uint64) == b.view(np.uint64)).all())}")
    vm.close()
    if out:
        with open(out, "a") as fh:
            fh.write("".join(LINES))


if __name__ == "__main__":
    main()
