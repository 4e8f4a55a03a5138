"""Option ks_fold_add on the GPU: y + rotate(x, o) as ONE key switch whose accumulators start at P . y (csrc/fused_ks.hip f_ks_frows_mac_kernel;
the rule: csrc/plan_exec.hip section 3a).  The addend enters and leaves exactly, so every limb is what "rotate, then add" gives:
  * dc_ct_rotate_hop_add against Oracle.add(Oracle.apply_galois(A, elt), Y), limb for limb, at N = 2^13 / 6 primes for every level, key, addend
    form and launch form of the middle, and at the reference size (N = 2^15, 14 primes, level 13);
  * programs through the plan (with its graph), the loop (plan = 0) and the oracle VM, option on and off: every result limb and scale equal, and
    the number of folds the plan reports equal to the number written beside each program."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from oracle.oracle import Ciphertext, Oracle, splitmix_fill  # noqa: E402
from gpu_helpers import _get_ct, _import_keys, _mirror_vm  # noqa: E402

pytestmark = pytest.mark.gpu

LOGN, K = 13, 6
SLOTS = 1 << (LOGN - 1)


# ---- kernel level ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    from dacapo_amd import lowlevel as ll

    o = Oracle(LOGN, K)
    o.keygen(seed=0x4845564D, galois_elts=[3, 2 * (1 << LOGN) - 1, pow(3, (1 << LOGN) // 2 - 4, 2 << LOGN)])
    ctx = ll.Context(LOGN, K)
    assert ctx.primes == o.primes
    return ll, ctx, o, {}


def _rand_ct(o, ell, seed):
    q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
    return np.stack([np.stack([splitmix_fill(seed + 7 * p + i, o.N) for i in range(ell)]) % q for p in range(2)])


def _edge(o, ct, pattern):
    """the first four coefficients of every limb of both polynomials: 0 where pattern is 0, q - 1 where it is 1"""
    for i in range(ct.shape[1]):
        for k, one in enumerate(pattern):
            ct[:, i, k] = np.uint64(o.primes[i] - 1) if one else np.uint64(0)
    return ct


def _case(o, cache, ell, elt):
    """source A, addend Y and the oracle's three results for a (level, key): computed once, shared by every launch form.  Y's first four
    coefficients are 0 / q - 1 like A's, and Y.c0 is also 0 / q - 1 exactly where galois(A.c0) is: both wraps of the kernel's addmod occur
    (q - 1 + q - 1 and 0 + 0 among them) wherever the automorphism sends A's edge coefficients."""
    key = (ell, elt)
    if key not in cache:
        a = _edge(o, _rand_ct(o, ell, 51 + ell), (0, 1, 0, 1))
        y = _edge(o, _rand_ct(o, ell, 61 + ell), (0, 1, 1, 0))
        g0 = o.galois_ntt(a[0], elt).reshape(ell, o.N)
        for i in range(ell):
            top = np.uint64(o.primes[i] - 1)
            y[0, i, g0[i] == top] = top
            y[0, i, g0[i] == 0] = 0
        A, Y = Ciphertext(a, 2.0**40), Ciphertext(y, 2.0**40)
        rot = o.apply_galois(A, elt)
        cache[key] = (a, y, o.add(rot, Y).data, o.add(rot, A).data, rot.data)
    return cache[key]


def _check_hop_add(ll, ctx, o, ell, elt, case, cap=None):
    L, N = ll.lib(), o.N
    cap = cap or o.K - 1
    a, y, want_other, want_self, rot = case
    st = cap * N

    def dev(ct):
        buf = np.zeros((2, cap, N), dtype=np.uint64)
        buf[:, :ell] = ct
        return ll.DeviceBuffer.from_host(buf)

    da, dy, dd, dk = dev(a), dev(y), ll.DeviceBuffer((2, cap, N)), ll.DeviceBuffer.from_host(o.galois[elt])
    L.dc_ct_rotate_hop_add(ctx.h, dd.ptr, st, da.ptr, st, dy.ptr, st, elt, dk.ptr, ell, None)  # another ciphertext
    assert (dd.to_host()[:, :ell] == want_other).all(), ("addend: another ciphertext", ell, elt)
    assert (da.to_host()[:, :ell] == a).all() and (dy.to_host()[:, :ell] == y).all()
    L.dc_ct_rotate_hop_add(ctx.h, dd.ptr, st, da.ptr, st, da.ptr, st, elt, dk.ptr, ell, None)  # the source itself: y' = y + rotate(y)
    assert (dd.to_host()[:, :ell] == want_self).all(), ("addend: the source", ell, elt)
    L.dc_ct_rotate_hop_add(ctx.h, dy.ptr, st, da.ptr, st, dy.ptr, st, elt, dk.ptr, ell, None)  # the addend is the destination
    assert (dy.to_host()[:, :ell] == want_other).all(), ("addend: the destination", ell, elt)
    L.dc_ct_rotate_hop(ctx.h, dd.ptr, st, da.ptr, st, elt, dk.ptr, ell, None)  # (and the plain hop beside it, on the same item slots)
    assert (dd.to_host()[:, :ell] == rot).all(), ("no addend", ell, elt)


@pytest.mark.parametrize("ell", [1, 2, 3, 5])
def test_rotate_hop_add_every_key(env, ell):
    ll, ctx, o, cache = env
    for elt in o.galois:
        _check_hop_add(ll, ctx, o, ell, elt, _case(o, cache, ell, elt))


@pytest.mark.parametrize("opts", [{"ks_merge_special_min_wgs": 0, "ks_merge_lift_min_wgs": 0}, {"small_tile_wgs": 0, "wide_tile_wgs": 0}])
def test_rotate_hop_add_launch_forms_l2(env, opts):
    """level 2 with the merged forms of the middle and the lift (one workgroup row for both special-prime accumulators: it gets no start
    value), and with the forced tile geometries"""
    from dacapo_amd import runner

    ll, ctx, o, cache = env
    with runner.options(**opts):
        for elt in o.galois:
            _check_hop_add(ll, ctx, o, 2, elt, _case(o, cache, 2, elt))


@pytest.fixture(scope="module")
def ref_size():
    """N = 2^15, 14 primes, level 13, one key: the oracle's results once for the three launch-shape sets"""
    o = Oracle(15, 14)
    o.keygen(seed=0x4845564D, galois_elts=[3], relin=False)
    return o, _case(o, {}, 13, 3)


@pytest.mark.parametrize("opts", [{}, {"small_tile_wgs": 0, "wide_tile_wgs": 0}, {"cols_pairs": 0, "tiny_tile_wgs": 512}])
def test_rotate_hop_add_reference_size_l13(ref_size, opts):
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    o, case = ref_size
    with runner.options(**opts):
        ctx = ll.Context(15, 14)
        _check_hop_add(ll, ctx, o, 13, 3, case, cap=13)


# ---- program level -----------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.ell == b.ell and a.scale == b.scale and bool((a.data == b.data).all())


def _res_regs(hv):
    from dacapo_amd import hevm_asm as ha

    return [int(r) for r in ha.unpack_hevm(hv)["res_dst"]]


class _VM:
    """a VM with options, the program loaded (trace kept) and the inputs set; run() returns the result registers' limbs per stream"""

    def __init__(self, cst, hv, args, opts, capfd, streams=1, launch_opts=None):
        from dacapo_amd import lowlevel as ll
        from dacapo_amd import runner

        self.ll, self.streams, self.regs, self.launch_opts = ll, streams, _res_regs(hv), launch_opts or {}
        self.hevm = runner.HEVM(seed=29, logN=LOGN, num_primes=K, vm_options=opts)
        if streams > 1:
            self.hevm.set_streams(streams)
        capfd.readouterr()
        with runner.options(trace=1, **self.launch_opts):
            self.hevm.load_mem(cst, hv)
        self.trace = "".join(line + "\n" for line in capfd.readouterr().err.splitlines() if "plan" in line and " ms" not in line)
        for s in range(streams):
            if streams > 1:
                self.hevm.select_stream(s)
            for i, a in enumerate(args):
                self.hevm.setInput(i, np.roll(a, 5 * s))

    def input_limbs(self, n):
        return [_get_ct(self.hevm, self.ll, i) for i in range(n)]

    def run(self):
        from dacapo_amd import runner

        with runner.options(**self.launch_opts):
            self.hevm.run()
        out = []
        for s in range(self.streams):
            if self.streams > 1:
                self.hevm.select_stream(s)
            out.append([_get_ct(self.hevm, self.ll, r) for r in self.regs])
        self.stats = self.hevm.stats()
        return out

    def close(self):
        self.hevm.close()


def _assert_equal_runs(a, b, what):
    assert len(a) == len(b)
    for s, (ra, rb) in enumerate(zip(a, b)):
        assert len(ra) == len(rb)
        for k, (x, y) in enumerate(zip(ra, rb)):
            assert _same(x, y), (what, "stream", s, "result", k)


def _builder(policy="eager"):
    from dacapo_amd import hevm_asm as ha

    return ha.Builder(slots=SLOTS, init_level=K - 1, policy=policy, shadow=True)


def _flush(b, v, n=16):
    """A register that still names a value when the program ends makes that value observable, and the plan keeps it as the program wrote
    it (nothing folds into or through it).  A long program recycles its registers; these short ones do it with `n` more results."""
    for _ in range(n):
        b.output(b.negate(v))


def _chains(offsets, chains=5):
    """`chains` independent reduction trees y' = y + rotate(y, o), stage by stage over `offsets`: the stages' rotations share steps"""
    rng = np.random.default_rng(41)
    b = _builder()
    ys = [b.input(rng.uniform(-1, 1, SLOTS)) for _ in range(chains)]
    for o in offsets:
        ys = [b.add(y, b.rotate(y, o)) for y in ys]
    for y in ys:
        b.output(y)
    _flush(b, ys[0])
    return b


def _prog_older_addend():
    """the addend is an older value that is not the rotation's source: a program input, and a value made two waves before the rotation starts"""
    rng = np.random.default_rng(42)
    b = _builder()
    x, w = b.input(rng.uniform(-1, 1, SLOTS)), b.input(rng.uniform(-1, 1, SLOTS))
    z1 = b.add(x, b.rotate(w, 1))
    n = b.negate(x)
    z2 = b.add(n, b.rotate(b.negate(b.negate(w)), 2))
    b.output(z1)
    b.output(z2)
    _flush(b, z1)
    return b


def _prog_mixed_step():
    """two rotations of one wave and level, one step: x + rotate(x, 1) folds, rotate(w, 1) is a result of its own and carries no addend"""
    rng = np.random.default_rng(43)
    b = _builder()
    x, w = b.input(rng.uniform(-1, 1, SLOTS)), b.input(rng.uniform(-1, 1, SLOTS))
    u = b.add(x, b.rotate(x, 1))
    v = b.rotate(w, 1)
    b.output(u)
    b.output(v)
    _flush(b, u)
    return b


def _prog_read_twice():
    rng = np.random.default_rng(44)
    b = _builder()
    x, w = b.input(rng.uniform(-1, 1, SLOTS)), b.input(rng.uniform(-1, 1, SLOTS))
    r = b.rotate(x, 1)
    b.output(b.add(x, r))
    b.output(b.add(r, w))
    _flush(b, x)
    return b


def _prog_three_terms():
    rng = np.random.default_rng(45)
    b = _builder()
    x, w = b.input(rng.uniform(-1, 1, SLOTS)), b.input(rng.uniform(-1, 1, SLOTS))
    t = b.add(b.add(x, b.rotate(x, 1)), w)
    b.output(t)
    _flush(b, t)
    return b


def _prog_plain_term():
    rng = np.random.default_rng(46)
    b = _builder()
    x, w = b.input(rng.uniform(-1, 1, SLOTS)), b.input(rng.uniform(-1, 1, SLOTS))
    wp = b.mul_plain(w, rng.uniform(-1, 1, SLOTS), normalise=False)
    t = b.add(b.mul_plain(x, rng.uniform(-1, 1, SLOTS), normalise=False), b.rotate(wp, 1))  # (the product is a term x * m of the sum)
    b.output(t)
    b.output(b.negate(wp))  # (a second reader keeps wp a value of its own)
    _flush(b, t)
    return b


def _prog_two_rotations_one_wave():
    rng = np.random.default_rng(47)
    b = _builder()
    x, w = b.input(rng.uniform(-1, 1, SLOTS)), b.input(rng.uniform(-1, 1, SLOTS))
    t = b.add(b.rotate(x, 1), b.rotate(w, 2))
    b.output(t)
    _flush(b, t)
    return b


def _prog_sum_read_by_rescale():
    rng = np.random.default_rng(48)
    b = _builder()
    x = b.input(rng.uniform(-1, 1, SLOTS))
    p = b.mul_plain(x, rng.uniform(-1, 1, SLOTS), normalise=False)  # (one prime above the waterline: the sum is what the rescale reads)
    r = b.rescale(b.add(p, b.rotate(p, 1)))
    b.output(r)
    _flush(b, r)
    return b


# (program, streams, launch-shape options in force at load and run, folds per run() with ks_fold_add = 1)
PROGRAMS = {
    "chains_1_2_4": (lambda: _chains((1, 2, 4)), 1, {}, 15),          # 5 chains x 3 stages, one hop each
    "chains_3_5_3": (lambda: _chains((3, 5, 3)), 1, {}, 15),          # 5 chains x 3 stages of two hops: the last hop carries the addend
    "older_addend": (_prog_older_addend, 1, {}, 2),
    "mixed_step": (_prog_mixed_step, 1, {}, 1),
    "two_streams": (lambda: _chains((1, 2, 4)), 2, {}, 30),           # every stream counted
    "read_twice": (_prog_read_twice, 1, {}, 0),
    "three_terms": (_prog_three_terms, 1, {}, 0),
    "plain_term": (_prog_plain_term, 1, {}, 0),
    "two_rotations_one_wave": (_prog_two_rotations_one_wave, 1, {}, 0),
    "sum_read_by_rescale": (_prog_sum_read_by_rescale, 1, {}, 0),
    "unfused_middle": (lambda: _chains((1, 2, 4), chains=2), 1, {"ks_fuse_mac": 0}, 0),  # the planner folds nothing, results unchanged
}


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_program_same_limbs_and_fold_count(name, capfd, tmp_path):
    from dacapo_amd import lowlevel as ll

    make, streams, launch_opts, folds = PROGRAMS[name]
    b = make()
    cst, hv, info = b.assemble()
    args = [a.plain for a in b.args]
    off = _VM(cst, hv, args, {"ks_fold_add": 0}, capfd, streams, launch_opts)
    o = Oracle(LOGN, K)
    _import_keys(o, off.hevm, ll, relin=False)
    ovm = _mirror_vm(off.hevm, ll, o, cst, hv, tmp_path)
    if streams > 1:  # (the oracle VM mirrors stream 0)
        off.hevm.select_stream(0)
    for i, c in enumerate(off.input_limbs(len(args))):
        ovm.ciphers[i] = c
    ref = off.run()
    st_off, trace_off = off.stats, off.trace
    off.close()
    assert st_off["add_folds"] == 0
    ovm.run()
    for k, r in enumerate(_res_regs(hv)):
        assert _same(ref[0][k], ovm.ciphers[r]), ("oracle VM", k)
    if streams == 1:  # (the loop runs one stream: with several, run() refuses plan = 0)
        loop = _VM(cst, hv, args, {"plan": 0}, capfd, 1, launch_opts)
        _assert_equal_runs(loop.run(), ref, "loop")
        assert loop.stats["add_folds"] == 0
        loop.close()
    on = _VM(cst, hv, args, {"ks_fold_add": 1}, capfd, streams, launch_opts)
    _assert_equal_runs(on.run(), ref, "ks_fold_add 1")
    _assert_equal_runs(on.run(), ref, "ks_fold_add 1, second run")
    print(f"{name}: add_folds {on.stats['add_folds']} (expected {folds}); keyswitches {on.stats['keyswitches']} ntts {on.stats['ntts']}")
    assert on.stats["add_folds"] == folds
    assert on.stats["ntts"] == st_off["ntts"] and on.stats["keyswitches"] == st_off["keyswitches"]
    if folds == 0:  # nothing folds: the plan is the one the option's 0 builds, line for line of the trace
        assert on.trace == trace_off
    else:
        assert "plan folds: %d two-term sums" % folds in on.trace and "plan folds" not in trace_off
    on.close()
