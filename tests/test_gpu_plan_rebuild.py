"""GPU: a plan rebuilt for ANOTHER program on a live VM (dacapo_amd/csrc/plan_exec.hip HEVM::release_plan / build_plan).  Loading a program
drops the plan; the next run() builds a new one, which first returns every table, arena and scratch the old one allocated and starts from
default counters.  Two programs of different shapes, A and B, alternate on ONE VM -- A, B, A, B, A, B -- under five option sets.  Between them
they fill every device table of a plan: rotations in one wave, an n-ary sum, a square whose rescale is linked to it, addcp / mulcp folded
into a rescale, a sum folded into a rescale, a negate, sums of ct x ct products (a relinearisation group under option ks_lazy_relin, a merged
multiply-rescale step under ks_fold_rescale) and one opcode 10; B has more items in every step than A, so every table and scratch is re-sized.
After every run the decrypted result meets the tolerance of test_gpu_hevm.py::test_destroy_returns_the_vms_memory (rms < 1e-5 against the
cleartext evaluation) and the run's counters equal those of a FRESH VM of the same options on that program: nothing of the previous plan
shows.  Device memory: free memory after the second B against free memory after the last B -- the same program is in place both times, so
a rebuild that forgets an arena or a lane's scratch shows as growth.  The bound is one lane's batch scratch for B.  That check is coarse: it
sees scratch, arenas and pool buffers, not a 100-byte item table, and the granularity at which the allocator reports free memory on these
devices has not been measured."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOGN, K = 12, 7
N, SLOTS, TOP = 1 << LOGN, 1 << (LOGN - 1), K - 1
B_TAPS = 8  # rotations of B's widest key-switch step (A: 3)


def _program(wide):
    from dacapo_amd import hevm_asm as ha

    rng = np.random.default_rng(5 if wide else 3)
    b = ha.Builder(slots=SLOTS, init_level=TOP, policy="lazy", boot_level=5, shadow=True)

    def pt(scale):
        return rng.uniform(-scale, scale, SLOTS)

    x = b.input(rng.uniform(-1, 1, SLOTS))
    if not wide:  # A: one input, three rotations
        r = [b.rotate(x, 1 << k) for k in range(3)]                            # one wave, one step
        s = b.add(b.add(r[0], r[1]), r[2])                                     # a three-term sum
        z = b.hint(b.mul(s, s), 0)                                             # a square and the rescale that alone reads it: a link
    else:  # B: two inputs, eight rotations, product sums
        y = b.input(rng.uniform(-1, 1, SLOTS))
        r = [b.rotate(x if k % 2 else y, 1 << k) for k in range(B_TAPS)]
        acc = None
        for t in r:                                                            # ct x pt products folded into their sum, the sum into its rescale
            term = b.mul_plain(t, pt(0.3))
            acc = term if acc is None else b.add(acc, term)
        bare = b.add(b.add(r[0], r[1]), b.add(r[2], r[3]))                     # a four-term sum of bare ciphertexts
        prods = b.sub(b.add(b.mul(bare, x), b.mul(y, y)), b.mul(x, y))         # + a b + c c - d e: three products, one negate
        s = b.add(b.hint(prods, 0), b.hint(acc, 0))
        z = b.hint(b.mul(s, s), 0)                                             # the linked square again, one level down
    f = b.hint(b.mul_plain(b.add_plain(z, pt(0.5)), pt(0.1)), 0)               # rescale((z + a) * m): both plaintexts folded in
    g = b.add(b.negate(f), b.rotate(f, 8))
    v = b.hint(g, 99)                                                          # opcode 10
    b.output(b.finish(b.mul_plain(v, pt(1.0))))
    if wide:
        b.output(b.finish(b.mul_plain(b.negate(g), pt(1.0))))
    cst, hv, info = b.assemble()
    assert info["op_mix"]["bootstrap"] == 1 and info["op_mix"]["negate"] >= 1
    return {"cst": cst, "hevm": hv, "inputs": [a.plain for a in b.args], "expected": b.expected()}


_PROGRAMS: dict = {}


def _programs():
    """A and B, assembled once and left unchanged"""
    if not _PROGRAMS:
        _PROGRAMS.update(A=_program(False), B=_program(True))
    return _PROGRAMS


def _free_bytes():
    from dacapo_amd import lowlevel as ll

    L = ll.lib()
    L.dc_mem_info.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.dc_mem_info.restype = None
    L.dc_device_sync()
    f, t = ctypes.c_uint64(), ctypes.c_uint64()
    L.dc_mem_info(ctypes.byref(f), ctypes.byref(t))
    return f.value


def _new_vm(opts, streams):
    from dacapo_amd import runner

    hevm = runner.HEVM(seed=77, logN=LOGN, num_primes=K, vm_options=opts)
    if streams > 1:
        hevm.set_streams(streams)
    return hevm


def _load_and_run(hevm, prog, streams):
    """load, encrypt every stream's inputs, run: (outputs per stream, counters)"""
    hevm.load_mem(prog["cst"], prog["hevm"])
    for q in range(streams):
        hevm.select_stream(q)
        for i, x in enumerate(prog["inputs"]):
            hevm.setInput(i, x)
    hevm.run()
    outs = []
    for q in range(streams):
        hevm.select_stream(q)
        outs.append(hevm.getOutput())
    hevm.select_stream(0)
    counters = {"stats": hevm.stats(), "hoist": hevm.hoist_stats(), "relin": hevm.relin_stats(), "fold": hevm.fold_rescale_stats(),
                "plaintext_bytes": hevm.plaintextBytes()}
    return outs, counters


@pytest.mark.parametrize("opts, streams", [
    ({}, 1),
    ({"online_encode": 1}, 1),
    ({"zenc_head": 0}, 1),
    ({"ks_fold_rescale": 1, "ks_lazy_relin": 1, "plan_level": 0}, 1),
    ({}, 2),
], ids=["default", "online_encode", "zenc_head0", "fold_relin_level0", "two_streams"])
def test_a_rebuilt_plan_owes_nothing_to_the_one_before(opts, streams):
    progs = _programs()
    fresh = {}
    for name, prog in progs.items():  # what a fresh VM of these options reports for each program
        vm = _new_vm(opts, streams)
        fresh[name] = _load_and_run(vm, prog, streams)[1]
        vm.close()
    if opts.get("ks_lazy_relin"):  # (the option set that is there for the product sums does group them)
        assert fresh["B"]["relin"]["groups"] >= 1 and fresh["B"]["fold"] >= 1
    hevm = _new_vm(opts, streams)
    free_after_b = []
    for rnd in range(3):
        for name in ("A", "B"):
            outs, counters = _load_and_run(hevm, progs[name], streams)
            for q, out in enumerate(outs):
                for got, want in zip(out, progs[name]["expected"]):
                    rms = float(np.sqrt(np.mean((got - want) ** 2)))
                    print(f"{name} round {rnd} stream {q}: rms {rms:.3e}")
                    assert rms < 1e-5, (name, rnd, q, rms)
            assert counters == fresh[name], (name, rnd)
            if name == "B":
                free_after_b.append(_free_bytes())
    hevm.close()
    # one lane's batch scratch (plan.hpp BatchWs) for B's widest key-switch step, B_TAPS rotations at TOP primes in one stream: target and
    # digits l limbs an item, the lifted digits l * l, the accumulators 2 (l + 1), the scratch 2 l -- of N words each
    lane_scratch = B_TAPS * (TOP + TOP + TOP * TOP + 2 * (TOP + 1) + 2 * TOP) * N * 8
    growth = free_after_b[1] - free_after_b[2]
    print(f"free after the second B {free_after_b[1]}, after the last B {free_after_b[2]}: growth {growth} bytes (bound {lane_scratch})")
    assert growth < lane_scratch, f"{growth / 1e6:.1f} MB more held after the last B than after the second"
