"""Option plan_level on the GPU: the slack-aware levelling of the plan (csrc/plan_levels.cpp) and the plaintext addend hoisted out of a rescale's
folded sum (csrc/plan_exec.hip section 2) move no arithmetic, so every limb of every result register is what the ASAP plan (plan_level = 0) and
the one-instruction-at-a-time loop (plan = 0) compute.  N = 2^12, 6 primes, the zero-encryption hook on (opcode 10 then leaves its re-encoded
plaintext in c0: deterministic), as tests/test_gpu_hevm.py does.  The oracle VM draws a fresh encryption in its opcode 10, so limbs are compared
with it where no opcode 10 lies upstream, and decoded values elsewhere."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from oracle.oracle import Oracle  # noqa: E402
from gpu_helpers import _get_ct, _import_keys, _mirror_vm  # noqa: E402

pytestmark = pytest.mark.gpu

LOGN, K = 12, 6
SLOTS = 1 << (LOGN - 1)
TRACE = re.compile(r"plan levels: plan_level (\d+) moved (\d+) operations: (\d+) steps in (\d+) waves, (\d+) waves with more than one step, "
                   r"(\d+) links, (\d+) step launches")
KIND_LINE = re.compile(r"plan:\s+(\w+)\s+(\d+) steps\s+(\d+) items")


def _same(a, b):
    return a.ell == b.ell and a.scale == b.scale and bool((a.data == b.data).all())


def _res_regs(hv):
    from dacapo_amd import hevm_asm as ha

    return [int(r) for r in ha.unpack_hevm(hv)["res_dst"]]


class _VM:
    """a VM with options, the program loaded and the inputs set; run() returns the result registers' limbs (per stream)"""

    def __init__(self, cst, hv, args, opts, capfd, streams=1):
        from dacapo_amd import lowlevel as ll
        from dacapo_amd import runner

        self.ll, self.streams, self.regs = ll, streams, _res_regs(hv)
        self.hevm = runner.HEVM(seed=29, logN=LOGN, num_primes=K, vm_options=opts)
        self.hevm.lw.hevm_test_zero_encryption(self.hevm.vm, True)
        if streams > 1:
            self.hevm.set_streams(streams)
        capfd.readouterr()
        with runner.options(trace=1):
            self.hevm.load_mem(cst, hv)
        err = capfd.readouterr().err
        m = TRACE.findall(err)
        self.fig = dict(zip(("level", "moved", "steps", "waves", "multi", "links", "launches"), (int(v) for v in m[-1]))) if m else None
        self.kinds = {k: (int(s), int(i)) for k, s, i in KIND_LINE.findall(err)}
        for s in range(streams):
            if streams > 1:
                self.hevm.select_stream(s)
            for i, a in enumerate(args):
                self.hevm.setInput(i, np.roll(a, 5 * s))

    def input_limbs(self, n):
        return [_get_ct(self.hevm, self.ll, i) for i in range(n)]

    def run(self):
        self.hevm.run()
        out = []
        for s in range(self.streams):
            if self.streams > 1:
                self.hevm.select_stream(s)
            out.append([_get_ct(self.hevm, self.ll, r) for r in self.regs])
        return out

    def close(self):
        self.hevm.close()


def _assert_equal_runs(a, b, what):
    assert len(a) == len(b)
    for s, (ra, rb) in enumerate(zip(a, b)):
        for k, (x, y) in enumerate(zip(ra, rb)):
            assert _same(x, y), (what, "stream", s, "result", k)


def _two_chain_program():
    """the hand-written shape of tests/test_plan_levels.py as a real program.  Lazy policy at 3-prime re-encryptions: the deep chain cycles
    multiply (3 primes) -> rescale -> multiply (2 primes) -> rescale -> opcode 10 -> ..., and the shallow chain -- a rotation, then three
    multiplies -- needs the same kinds at the same levels, a few waves after ASAP would run them alone; it joins the deep chain by an add near
    the end.  Outputs: the joined result, and the rotation's first product (no opcode 10 upstream: compared with the oracle VM limb for limb)."""
    from dacapo_amd import hevm_asm as ha

    rng = np.random.default_rng(17)
    b = ha.Builder(slots=SLOTS, init_level=3, policy="lazy", boot_level=3, shadow=True)
    x, y = b.input(rng.uniform(0.7, 1.0, SLOTS)), b.input(rng.uniform(0.7, 1.0, SLOTS))
    t = x
    for _ in range(11):
        t = b.mul(t, x)
    s = b.rotate(y, 3)
    s1 = b.mul(s, y)
    s = b.mul(b.mul(s1, y), y)
    r = b.mul(b.add(t, s), y)
    b.output(b.finish(r))
    b.output(b.finish(s1))
    return b


@pytest.fixture(scope="module")
def two_chain():
    b = _two_chain_program()
    cst, hv, info = b.assemble()
    assert info["op_mix"]["bootstrap"] >= 3 and info["op_mix"]["rescale"] >= 8
    return b, cst, hv


def test_two_chain_program_fewer_steps_same_limbs_in_every_execution_form(two_chain, capfd, tmp_path):
    """(a) plan_level 0 and 1 and the loop give identical limbs on every result register, under plan_graph 0 / 1 / 2 and plan_lanes 1 / 2;
    the re-levelled plan has fewer steps, no more waves and fewer launches than the ASAP plan (from the trace)."""
    from dacapo_amd import lowlevel as ll

    b, cst, hv = two_chain
    args = [a.plain for a in b.args]
    ref_vm = _VM(cst, hv, args, {"plan_level": 0}, capfd)
    o = Oracle(LOGN, K)
    _import_keys(o, ref_vm.hevm, ll)
    ovm = _mirror_vm(ref_vm.hevm, ll, o, cst, hv, tmp_path)
    for i, c in enumerate(ref_vm.input_limbs(len(args))):
        ovm.ciphers[i] = c
    ref = ref_vm.run()
    out = ref_vm.hevm.getOutput()
    fig0 = ref_vm.fig
    ref_vm.close()
    assert fig0 and fig0["level"] == 0 and fig0["moved"] == 0
    loop = _VM(cst, hv, args, {"plan": 0}, capfd)
    _assert_equal_runs(loop.run(), ref, "loop")
    loop.close()
    for graph in (0, 1, 2):
        for lanes in (1, 2):
            vm = _VM(cst, hv, args, {"plan_level": 1, "plan_graph": graph, "plan_lanes": lanes}, capfd)
            fig1 = vm.fig
            print(f"plan_graph {graph} plan_lanes {lanes}: plan_level 0 {fig0}  plan_level 1 {fig1}")
            assert fig1 and fig1["level"] == 1 and fig1["moved"] > 0
            assert fig1["steps"] < fig0["steps"] and fig1["waves"] <= fig0["waves"] and fig1["launches"] < fig0["launches"], (fig0, fig1)
            _assert_equal_runs(vm.run(), ref, (graph, lanes))
            _assert_equal_runs(vm.run(), ref, (graph, lanes, "second run"))
            vm.close()
    # the oracle VM: limb for limb where no opcode 10 lies upstream; decoded values (its opcode 10 draws a fresh encryption) for the joined
    # result, to the bound tests/test_gpu_hevm.py sets for lazy programs with opcode 10 (rms 2e-5 of the peak), and the cleartext shadow too
    ovm.run()
    want = ovm.ciphers[_res_regs(hv)[1]]
    assert _same(ref[0][1], want)
    dec = o.decode(o.decrypt(ovm.ciphers[_res_regs(hv)[0]]))
    for refv in (np.real(dec)[:SLOTS], b.expected()[0]):
        assert np.sqrt(np.mean((out[0][:SLOTS] - refv[:SLOTS]) ** 2)) < 2e-5 * max(1.0, float(np.abs(refv).max()))


@pytest.mark.parametrize("seed", [100, 101])
def test_resnet_shaped_layers_same_limbs(capfd, seed):
    """(b) two layers of the ResNet-shaped program (convolution taps, rotate-and-sum, addcp chain, activation with opcode 10): plan_level 0
    against 1, limb for limb, run twice each.  (Lowered eagerly, these two layers are one dependency chain -- 210 steps in 210 waves -- so the
    pass finds nothing to move here: the case pins that a plan without slack comes out unchanged and still runs under the option.)"""
    from dacapo_amd import hevm_asm as ha

    # (2^11 slots: an offset below 2^10 has at most 5 non-adjacent digits, so the default tap list's 6-hop offset cannot be drawn; a shorter
    # list with the same spread of 1 .. 4 hops keeps the program small)
    b = ha.resnet_shaped(seed=seed, slots=SLOTS, layers=2, init_level=K - 1, shadow=True, tap_hops=[1] * 14 + [2] * 3 + [3] * 2 + [4])
    cst, hv, _ = b.assemble()
    args = [a.plain for a in b.args]
    runs = {}
    for level in (0, 1):
        vm = _VM(cst, hv, args, {"plan_level": level}, capfd)
        print(f"resnet_shaped seed {seed} plan_level {level}: {vm.fig} {vm.kinds}")
        runs[level] = (vm.run(), vm.run(), vm.fig)
        vm.close()
        _assert_equal_runs(runs[level][0], runs[level][1], ("second run", level))
    _assert_equal_runs(runs[0][0], runs[1][0], "plan_level 1 against 0")
    assert runs[1][2]["steps"] <= runs[0][2]["steps"] and runs[1][2]["waves"] <= runs[0][2]["waves"]


def test_three_streams_same_limbs(two_chain, capfd):
    """(c) three ciphertext streams through one plan (a step's chunk is max_batch / 3 items): every stream's limbs under plan_level 1 equal
    those under plan_level 0"""
    b, cst, hv = two_chain
    args = [a.plain for a in b.args]
    runs = {}
    for level in (0, 1):
        vm = _VM(cst, hv, args, {"plan_level": level}, capfd, streams=3)
        runs[level] = vm.run()
        vm.close()
    assert len(runs[0]) == 3 and not _same(runs[0][0][0], runs[0][1][0])  # (the streams do carry different data)
    _assert_equal_runs(runs[1], runs[0], "three streams")


def _hoist_program(case):
    """a rescale of  sum_k x_k * m_k + (y * m + a):  "plain": plaintexts at one prime's worth of scale; "upscaled": plaintexts at the waterline and
    an outer all-ones mulcp in front of the rescale (folded as the rescale's multiplier); "two": two addcp terms, of which one may hoist"""
    from dacapo_amd import hevm_asm as ha

    rng = np.random.default_rng(23)
    b = ha.Builder(slots=SLOTS, init_level=3, policy="eager", shadow=True)
    xs = [b.input(rng.uniform(-1, 1, SLOTS)) for _ in range(4)]
    bits = 40 if case == "upscaled" else 60
    acc = None
    for x in xs[:2]:
        t = b.mul_plain(x, rng.uniform(-1, 1, SLOTS), scale_bits=bits, normalise=False)
        acc = t if acc is None else b.add(acc, t)
    for y in xs[2:] if case == "two" else xs[2:3]:
        t = b.add_plain(b.mul_plain(y, rng.uniform(-1, 1, SLOTS), scale_bits=bits, normalise=False), rng.uniform(-1, 1, SLOTS))
        acc = b.add(acc, t)
    if case == "upscaled":
        acc = b.upscale(acc, 20)
    r = b.rescale(acc)
    b.output(r)
    # A register that still names the addcp's result when the program ends makes that result observable (the plan pins it), and nothing folds.
    # A long program recycles its registers; this short one does it with three more results, which take the registers the sum has freed.
    for _ in range(3):
        b.output(b.negate(r))
    return b


@pytest.mark.parametrize("case", ["plain", "upscaled", "two"])
def test_addend_hoisted_out_of_a_rescales_sum(capfd, tmp_path, case):
    """(d) the hoist: limbs equal to the oracle VM's and the loop's, with the levelling (plan_level 1) and alone (2); the trace shows the addcp
    and the mulcp behind it gone as steps (with two addcp terms, one of the two)"""
    from dacapo_amd import lowlevel as ll

    b = _hoist_program(case)
    cst, hv, _ = b.assemble()
    args = [a.plain for a in b.args]
    base = _VM(cst, hv, args, {"plan_level": 0}, capfd)
    o = Oracle(LOGN, K)
    _import_keys(o, base.hevm, ll)
    ovm = _mirror_vm(base.hevm, ll, o, cst, hv, tmp_path)
    for i, c in enumerate(base.input_limbs(len(args))):
        ovm.ciphers[i] = c
    ref, kinds0 = base.run(), base.kinds
    base.close()
    ovm.run()
    assert _same(ref[0][0], ovm.ciphers[_res_regs(hv)[0]])
    n_add = 2 if case == "two" else 1
    assert kinds0.get("addp") == (1, n_add) and kinds0.get("mulp") == (1, n_add), kinds0
    loop = _VM(cst, hv, args, {"plan": 0}, capfd)
    _assert_equal_runs(loop.run(), ref, "loop")
    loop.close()
    for level in (1, 2):
        vm = _VM(cst, hv, args, {"plan_level": level}, capfd)
        _assert_equal_runs(vm.run(), ref, ("plan_level", level))
        if case == "two":
            assert vm.kinds.get("addp") == (1, 1) and vm.kinds.get("mulp") == (1, 1), vm.kinds
        else:
            assert "addp" not in vm.kinds and "mulp" not in vm.kinds, vm.kinds
        vm.close()
