"""GPU: the three-part ciphertext at the kernel-level ABI and lazy relinearisation (include/dacapo_ckks.h dc_ct_mul, dc_ct_relin,
dc_ct_mul_sum_relin; dacapo_amd/csrc/fused_ks.hip f_irows_tensor_sum_kernel / f_frows_sum_final_kernel, batch_ops.hip b_mul_sum_relin).

Everything is compared limb for limb (==) with the unchanged oracle:
  * dc_ct_mul == Oracle.tensor; dc_ct_relin(dc_ct_mul(a, b)) == dc_ct_mul_relin(a, b) == Oracle.mul_relin(a, b);
  * dc_ct_mul_sum_relin == the definition: T = sum_k s_k Oracle.tensor(a_k, b_k) by poly_add / poly_sub, then Oracle.keyswitch(T2, relin, T0, T1),
    for 1, 2, 3 and the largest count of products with mixed signs; one product with sign + is dc_ct_mul_relin exactly;
  * a square, an operand shared by several terms, the destination being an operand;
  * every limb of every operand q_i - 1 at the largest count, signs all +, alternating, and + + -: the accumulators at their bound;
  * every forced launch shape at N = 2^12 (the tile geometries, the merged forms, the large-batch sequence, the un-fused middle with its
    tensor-sum launch).
VM level (option ks_lazy_relin): a program with two groups and three near-misses in three execution modes and two streams against an oracle
replay of the exported groups; the loop; the suite programs that hold groups.
Levels 1, 2, 3, 5 of a 6-prime chain at N = 2^12 and level 13 of the reference ring.  Inputs are uniform random limbs: the identities are
polynomial identities and need no ciphertexts."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.oracle import Ciphertext, Oracle, splitmix_fill  # noqa: E402

CAP = 32  # DC_CT_MUL_SUM_MAX (include/dacapo_ckks.h)
LEVELS = [(12, 6, 1), (12, 6, 2), (12, 6, 3), (12, 6, 5), (15, 14, 13)]

_RINGS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _release_rings_after_the_module():
    yield
    _RINGS.clear()
    gc.collect()


def _ring(logN, K):
    """oracle with a relinearisation key (host and device) and a context, made once per ring and left unchanged; the last entry caches the
    oracle's results"""
    from dacapo_amd import lowlevel as ll

    if (logN, K) not in _RINGS:
        o = Oracle(logN, K)
        o.keygen(seed=0x4845564D, galois_elts=[], relin=True)
        ctx = ll.Context(logN, K)
        assert ctx.primes == o.primes
        _RINGS[(logN, K)] = (o, ll.DeviceBuffer.from_host(o.relin), ctx, {})
    return _RINGS[(logN, K)]


def _operand(o, ell, which):
    """operand `which` of the level's pool: uniform limbs; which = "max": every limb q_i - 1"""
    q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
    if which == "max":
        return np.ascontiguousarray(np.broadcast_to((q - np.uint64(1))[None], (2, ell, o.N)))
    return np.stack([np.stack([splitmix_fill(1000 * which + 7 * p + i + 100 * ell, o.N) for i in range(ell)]) % q for p in range(2)])


def _terms(count, pool=4):
    """`count` terms (a, b, sign) over a pool of operands: (0,1) (1,3) -(2,1) (3,3) ... -- operands that several terms share from two terms
    on, a negative term from three on, a square from four on"""
    out = []
    for k in range(count):
        a, b = k % pool, (2 * k + 1) % pool
        out.append((a, b, -1 if k % 3 == 2 else 1))
    return out


def _define(ring, ell, terms):
    """the definition on the oracle, cached per (level, terms)"""
    o, cache = ring[0], ring[3]
    key = (ell, tuple(terms))
    if key not in cache:
        T = np.zeros((3, ell, o.N), dtype=np.uint64)
        for a, b, s in terms:
            t = o.tensor(Ciphertext(_operand(o, ell, a), 1.0), Ciphertext(_operand(o, ell, b), 1.0))
            T = np.stack([(o.poly_add if s > 0 else o.poly_sub)(T[p], t[p]) for p in range(3)])
        c0, c1 = T[0].copy(), T[1].copy()
        o.keyswitch(T[2], o.relin, c0, c1)
        cache[key] = np.stack([c0, c1])
    return cache[key]


def _call_sum(ring, ell, terms, dst=None):
    """dc_ct_mul_sum_relin over the pool's operands -> (result, the operands read back afterwards); dst: the operand that is the destination"""
    from dacapo_amd import lowlevel as ll

    o, dkey, ctx, _ = ring
    st = ell * o.N
    names = sorted({t[0] for t in terms} | {t[1] for t in terms}, key=str)
    dev = {w: ll.DeviceBuffer.from_host(_operand(o, ell, w)) for w in names}
    dd = dev[dst] if dst is not None else ll.DeviceBuffer((2, ell, o.N))
    ctx.mul_sum_relin(dd.ptr, st, [dev[t[0]].ptr for t in terms], [dev[t[1]].ptr for t in terms], [t[2] for t in terms], st, dkey.ptr, ell)
    ctx.L.dc_stream_sync(None)
    return dd.to_host(), {w: dev[w].to_host() for w in names if w != dst}


@pytest.mark.parametrize("logN,K,ell", LEVELS)
def test_mul_and_relin_are_the_two_halves_of_mul_relin(logN, K, ell):
    """dc_ct_mul == Oracle.tensor; dc_ct_relin of it == dc_ct_mul_relin == Oracle.mul_relin; relinearising in place gives the same"""
    from dacapo_amd import lowlevel as ll

    o, dkey, ctx, _ = ring = _ring(logN, K)
    N, L, st = o.N, ctx.L, ell * o.N
    a, b = _operand(o, ell, 0), _operand(o, ell, 1)
    da, db = ll.DeviceBuffer.from_host(a), ll.DeviceBuffer.from_host(b)
    d3, d2, dm = ll.DeviceBuffer((3, ell, N)), ll.DeviceBuffer((2, ell, N)), ll.DeviceBuffer((2, ell, N))
    L.dc_ct_mul(ctx.h, d3.ptr, st, da.ptr, st, db.ptr, st, ell, None)
    L.dc_ct_relin(ctx.h, d2.ptr, st, d3.ptr, st, dkey.ptr, ell, None)
    L.dc_ct_mul_relin(ctx.h, dm.ptr, st, da.ptr, st, db.ptr, st, dkey.ptr, ell, None)
    L.dc_stream_sync(None)
    t3 = d3.to_host()
    assert (t3 == o.tensor(Ciphertext(a, 1.0), Ciphertext(b, 1.0))).all()
    want = _define(ring, ell, [(0, 1, 1)])
    assert (want == o.mul_relin(Ciphertext(a, 1.0), Ciphertext(b, 1.0)).data).all()  # (the definition's anchor, on the oracle itself)
    assert (d2.to_host() == want).all() and (dm.to_host() == want).all()
    L.dc_ct_relin(ctx.h, d3.ptr, st, d3.ptr, st, dkey.ptr, ell, None)
    L.dc_stream_sync(None)
    inplace = d3.to_host()
    assert (inplace[:2] == want).all() and (inplace[2] == t3[2]).all()
    assert (da.to_host() == a).all() and (db.to_host() == b).all()


@pytest.mark.parametrize("logN,K,ell,count", [(12, 6, ell, n) for ell in (1, 2, 3, 5) for n in (1, 2, 3, CAP)] + [(15, 14, 13, 3)])
def test_mul_sum_relin_equals_the_definition(logN, K, ell, count):
    """mixed signs from three terms on; the largest count holds squares and operands that many terms share.  The operands are unchanged."""
    ring = _ring(logN, K)
    terms = _terms(count)
    got, ops = _call_sum(ring, ell, terms)
    assert (got == _define(ring, ell, terms)).all()
    for w, v in ops.items():
        assert (v == _operand(ring[0], ell, w)).all()


@pytest.mark.parametrize("ell", [1, 3])
def test_one_product_is_mul_relin(ell):
    """count = 1, sign +: dc_ct_mul_relin's limbs exactly -- the anchor to SEAL's own rounding; sign -: its negation's key switch"""
    from dacapo_amd import lowlevel as ll

    o, dkey, ctx, _ = ring = _ring(12, 6)
    st = ell * o.N
    got, _ = _call_sum(ring, ell, [(0, 1, 1)])
    da, db = ll.DeviceBuffer.from_host(_operand(o, ell, 0)), ll.DeviceBuffer.from_host(_operand(o, ell, 1))
    dm = ll.DeviceBuffer((2, ell, o.N))
    ctx.L.dc_ct_mul_relin(ctx.h, dm.ptr, st, da.ptr, st, db.ptr, st, dkey.ptr, ell, None)
    ctx.L.dc_stream_sync(None)
    assert (got == dm.to_host()).all()
    got, _ = _call_sum(ring, ell, [(0, 1, -1)])
    assert (got == _define(ring, ell, [(0, 1, -1)])).all()


@pytest.mark.parametrize("ell", [2, 3])
def test_squares_shared_operands_and_an_aliased_destination(ell):
    ring = _ring(12, 6)
    for terms, dst in [([(0, 0, 1), (1, 1, -1)], None),             # squares: a_k is b_k
                       ([(0, 1, 1), (0, 2, 1), (2, 0, -1)], None),   # one operand in every term, on either side
                       ([(0, 1, 1), (2, 3, -1)], 0),                 # dst is an a operand
                       ([(0, 1, 1), (2, 3, -1), (3, 3, 1)], 3),      # dst is a b operand and both sides of a square
                       ([(0, 0, 1)], 0)]:                            # one square onto itself
        got, ops = _call_sum(ring, ell, terms, dst=dst)
        assert (got == _define(ring, ell, terms)).all(), (terms, dst)
        for w, v in ops.items():
            assert (v == _operand(ring[0], ell, w)).all(), (terms, dst, w)


@pytest.mark.parametrize("signs", ["plus", "alternating", "two_to_one"])
@pytest.mark.parametrize("ell", [1, 5])
def test_extreme_operands_at_the_largest_count(ell, signs):
    """every limb of every operand q_i - 1, CAP terms: each 128-bit accumulator takes the most it can between two folds (16 products of
    (q - 1)^2 on the c1 component) -- all in one accumulator, or split between the two signs' accumulators.  Alternating signs of equal terms
    cancel to zero whatever the two accumulators hold, as long as they hold the same; + + - does not."""
    ring = _ring(12, 6)
    period = {"plus": 1, "alternating": 2, "two_to_one": 3}[signs]
    terms = [("max", "max", -1 if (period > 1 and k % period == period - 1) else 1) for k in range(CAP)]
    got, _ = _call_sum(ring, ell, terms)
    assert (got == _define(ring, ell, terms)).all()


@pytest.mark.parametrize("opts", [dict(tiny_tile_wgs=0, small_tile_wgs=0), dict(tiny_tile_wgs=0, small_tile_wgs=1 << 30), dict(tiny_tile_wgs=100000),
                                  dict(tiny_tile_wgs=0, small_tile_wgs=0, wide_tile_wgs=0, ks_big_tiles=0), dict(wide_tile_wgs=-1, ks_big_tiles=0),
                                  dict(ks_fuse_mac=0), dict(ks_fuse_mac=1), dict(ks_items_fast=0), dict(ks_items_fast=1),
                                  dict(ks_big_tiles=0, ks_merge_lift_min_wgs=0), dict(tiny_tile_wgs=0, ks_merge_lift_min_wgs=0),
                                  dict(ks_merge_special_min_wgs=0), dict(ks_merge_special_min_wgs=0, tiny_tile_wgs=0),
                                  dict(ks_big_tiles=1), dict(ks_fuse_mac_tiles=0), dict(ks_merge_lift_min_wgs=0, ks_merge_special_min_wgs=0)])
def test_under_every_forced_launch_shape(opts):
    """N = 2^12, l = 3: the launch-shape sets of tests/test_gpu_ks_fold_rescale.py.  Every tile geometry of the term-walking loaders, and the
    tensor-sum launch with the mode-1 form of the last kernel where the middle is not fused; an aliased destination under each as well."""
    from dacapo_amd import runner

    ring = _ring(12, 6)
    few, many = _terms(3), _terms(CAP)
    with runner.options(**opts):
        got3, _ = _call_sum(ring, 3, few)
        gotn, _ = _call_sum(ring, 3, many)
        gota, _ = _call_sum(ring, 3, few, dst=0)
    assert (got3 == _define(ring, 3, few)).all(), opts
    assert (gotn == _define(ring, 3, many)).all(), opts
    assert (gota == _define(ring, 3, few)).all(), opts


# ---- VM level (option ks_lazy_relin) -----------------------------------------------------------------------------------------------------
class _ThreePart:
    """a three-part ciphertext of the replay: [3][level][N] limbs and the scale label"""

    def __init__(self, data, scale):
        self.data, self.scale = data, scale


def _replay_vm(o):
    from oracle.oracle import OracleVM

    class Replay(OracleVM):
        """OracleVM that replays the plan's exported groups (hevm_plan_relin_groups): a member mulcc leaves Oracle.tensor's three parts, negate
        and addcc act on all three (addcc takes its rhs scale, as on two-part values), and the group's closing instruction finishes with ONE
        Oracle.keyswitch.  The grouping DECISION is the plan's; the arithmetic is the oracle's own."""
        members, closing = frozenset(), frozenset()

        def set_relin_groups(self, groups):
            self.members = frozenset(m for _, ms in groups for m, _ in ms)
            self.closing = frozenset(c for c, _ in groups)

        def step(self, op, index=None):
            oo, c = self.o, self.ciphers
            opcode, dst, lhs, rhs = (int(x) for x in op)
            if opcode == 8 and index in self.members:
                c[dst] = _ThreePart(oo.tensor(c[lhs], c[rhs]), c[lhs].scale * c[rhs].scale)
            elif opcode == 2 and isinstance(c[lhs], _ThreePart):
                c[dst] = _ThreePart(np.stack([oo.poly_neg(p) for p in c[lhs].data]), c[lhs].scale)
            elif opcode == 6 and (isinstance(c[lhs], _ThreePart) or isinstance(c[rhs], _ThreePart)):
                assert isinstance(c[lhs], _ThreePart) and isinstance(c[rhs], _ThreePart), f"op {index} adds a three-part value to a ciphertext"
                c[lhs].scale = c[rhs].scale
                c[dst] = _ThreePart(np.stack([oo.poly_add(a, b) for a, b in zip(c[lhs].data, c[rhs].data)]), c[rhs].scale)
            else:
                for r in ((lhs,) if opcode in (1, 2, 3, 4, 7, 9, 10) else (lhs, rhs) if opcode in (6, 8) else ()):
                    assert not isinstance(c[r], _ThreePart), f"op {index} (opcode {opcode}) reads an unfinished three-part value"
                super().step(op, index)
                return
            if index in self.closing:
                t = c[dst]
                c0, c1 = t.data[0].copy(), t.data[1].copy()
                oo.keyswitch(t.data[2], oo.relin, c0, c1)
                c[dst] = Ciphertext(np.stack([c0, c1]), t.scale)

    return Replay(o)


def _vm_program(slots, seed=29):
    """-> (builder, the two groups the plan must find as [(closing instruction, [(mulcc instruction, sign), ...])]):
    x y + z w - u u (an output); x z + y w + u x feeding a rescale; a product with two readers (an addcc and a negate); a product that is an
    output and is added to another; one product plus a ciphertext that is no product"""
    from dacapo_amd import hevm_asm as ha

    rng = np.random.default_rng(seed)
    b = ha.Builder(slots=slots, init_level=5, policy="eager", shadow=True)
    x, y, z, w, u, cc = [b.input(rng.uniform(-1, 1, slots)) for _ in range(6)]

    def mul(p, q):
        v = b.mul(p, q)
        return v, len(b.ops) - 1

    xy, i_xy = mul(x, y)
    zw, i_zw = mul(z, w)
    uu, i_uu = mul(u, u)
    g1 = b.sub(b.add(xy, zw), uu)
    c1 = len(b.ops) - 1
    b.output(g1)
    xz, i_xz = mul(x, z)
    yw, i_yw = mul(y, w)
    ux, i_ux = mul(u, x)
    g2 = b.add(b.add(xz, yw), ux)
    c2 = len(b.ops) - 1
    b.output(b.rescale(g2))
    p, _ = mul(x, w)                       # two readers
    b.output(b.add(p, mul(y, u)[0]))
    b.output(b.negate(p))
    m, _ = mul(z, u)                       # the product itself is an output
    b.output(m)
    b.output(b.add(m, mul(w, w)[0]))
    b.output(b.add(mul(y, z)[0], cc))      # a tree with a leaf that is no product (the builder brings cc to the product's scale with a mulcp)
    want = [(c1, [(i_xy, 1), (i_zw, 1), (i_uu, -1)]), (c2, [(i_xz, 1), (i_yw, 1), (i_ux, 1)])]
    for c, ms in want:
        assert int(b.ops[c].opcode) == ha.OP_ADDCC and all(int(b.ops[i].opcode) == ha.OP_MULCC for i, _ in ms)
    return b, want


def _run_vm(tmp_path, lazy, plan=1, graph=1, streams=1):
    """the program under ks_lazy_relin = lazy: every result register of every stream == the replay (lazy) / the plain OracleVM (off) on the
    same key / plaintext / input limbs -> (exported groups, stats, relin stats, max slot error per output of stream 0)"""
    from gpu_helpers import _get_ct, _import_keys, _mirror_vm

    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    logN, K = 12, 6
    hevm = runner.HEVM(seed=91, logN=logN, num_primes=K, vm_options={"plan": plan, "plan_graph": graph, "ks_lazy_relin": lazy})
    o = Oracle(logN, K)
    _import_keys(o, hevm, ll)
    if streams > 1:
        hevm.set_streams(streams)
    b, want_groups = _vm_program(1 << (logN - 1))
    cst, hv, _ = b.assemble()
    hevm.load_mem(cst, hv)
    ovms = []
    for s in range(streams):
        hevm.select_stream(s)
        base = _mirror_vm(hevm, ll, o, cst, hv, tmp_path)
        ovm = _replay_vm(o)
        ovm.load(tmp_path / "p.cst", tmp_path / "p.hevm")
        ovm.plains = base.plains
        for i, a in enumerate(b.args):
            hevm.setInput(i, a.plain * (1.0 - 0.25 * s))
            ovm.ciphers[i] = _get_ct(hevm, ll, i)
        ovms.append(ovm)
    before = hevm.relin_groups()
    hevm.run()
    groups = hevm.relin_groups()
    for s, ovm in enumerate(ovms):
        hevm.select_stream(s)
        if isinstance(groups, list):
            ovm.set_relin_groups(groups)
        ovm.run()
        assert len(ovm.prog.res_dst) == 7
        for r in ovm.prog.res_dst:
            got, want = _get_ct(hevm, ll, r), ovm.ciphers[r]
            assert got.ell == want.ell and got.scale == want.scale, (s, r)
            assert (got.data == want.data).all(), (s, r)
    hevm.select_stream(0)
    errs = [float(np.abs(got - want).max()) for got, want in zip(hevm.getOutput(), b.expected())]
    st, rst = hevm.stats(), hevm.relin_stats()
    hevm.close()
    return before, groups, want_groups, st, rst, errs


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("plan,graph", [(1, 1), (1, 0), (1, 2)])
def test_vm_groups_limbs_scale_and_error(tmp_path, plan, graph, streams):
    """option on: exactly the two groups, with their signs; every result's limbs and scale == the oracle replay of those groups; two key
    switches fewer per group of three; per output the maximum slot error against the cleartext result within 2 x the option-off run's (one key
    switch's noise replaces three; the factor covers the spread of a maximum over 2 048 slots).  Option off: limbs == the plain OracleVM,
    no groups, no counts."""
    before, groups, want, st, rst, errs = _run_vm(tmp_path, 1, plan, graph, streams)
    assert groups == want
    assert rst == {"groups": 2 * streams, "products": 6 * streams}
    b0, g0, _, st0, rst0, errs0 = _run_vm(tmp_path, 0, plan, graph, streams)
    assert g0 == 0 and rst0 == {"groups": 0, "products": 0}
    assert st["op_counts"] == st0["op_counts"] and st["op_counts"][8] == 11  # op_counts stay per instruction
    assert st0["keyswitches"] - st["keyswitches"] == 4 * streams and st["ntts"] < st0["ntts"]
    for k, (e1, e0) in enumerate(zip(errs, errs0)):
        assert e1 <= 2 * e0, f"output {k}: lazy {e1:.3e} against default {e0:.3e} (bound 2 x)"


def test_vm_loop_ignores_the_option(tmp_path):
    """plan = 0: the one-instruction-at-a-time loop runs every mulcc as it is (limbs == the plain OracleVM) and there is no plan to export"""
    before, groups, _, st, rst, _ = _run_vm(tmp_path, 1, plan=0)
    assert before == -1 and groups == -1 and rst == {"groups": 0, "products": 0}


@pytest.fixture(scope="module")
def suite_vms():
    from gpu_helpers import _import_keys  # noqa: F401

    from dacapo_amd import runner

    vms = {lazy: runner.HEVM(seed=0x4845564D + 2, logN=15, num_primes=14, vm_options={"ks_lazy_relin": lazy}) for lazy in (0, 1)}
    yield vms
    for vm in vms.values():
        vm.close()


# (closing instruction, [(mulcc instruction, sign), ...]) per group of the committed programs, as the stand-alone pass prints them
# (plan_groups_asan relin): recorded literals, so that the list the library exports is held to a record and not to the library
SUITE_GROUPS = {"Multivariate": [(1042, [(1032, 1), (1036, 1), (1040, 1)]), (1421, [(1413, 1), (1416, 1), (1419, 1)]),
                                 (1797, [(1789, 1), (1792, 1), (1795, 1)])],
                "HarrisCornerDetection": [(189, [(180, 1), (188, 1)])],
                "SobelFilter": [(68, [(65, 1), (67, 1)])]}


@pytest.mark.parametrize("name,sizes", [("Multivariate", [3, 3, 3]), ("HarrisCornerDetection", [2]), ("SobelFilter", [2])])
def test_suite_programs_group_as_the_static_pass_says(suite_vms, name, sizes):
    """the committed suite programs with groups: the exported list -- closing instruction, products, signs -- is the stand-alone pass's
    (tests/test_plan_relin.py), one key switch fewer per saved product, and the rms against the fixture's cleartext result within 2 x the
    option-off run's"""
    from pathlib import Path

    from dacapo_amd import hevm_asm as ha

    fx = ha.read_fixture(Path(__file__).resolve().parent / "golden" / "suite" / name)
    rms, ks = {}, {}
    for lazy, hevm in suite_vms.items():
        hevm.load_mem(fx["cst"], fx["hevm"])
        for i, x in enumerate(fx["inputs"]):
            hevm.setInput(i, x)
        hevm.run()
        rms[lazy] = float(np.sqrt(np.mean((hevm.getOutput() - fx["expected"]) ** 2)))
        ks[lazy] = hevm.stats()["keyswitches"]
        groups = hevm.relin_groups()
        if lazy:
            assert groups == SUITE_GROUPS[name] and [len(ms) for _, ms in groups] == sizes
            assert hevm.relin_stats() == {"groups": len(sizes), "products": sum(sizes)}
        else:
            assert groups == 0
    print(f"{name}: rms vs cleartext evaluation, ks_lazy_relin on {rms[1]:.3e}, off {rms[0]:.3e}; key switches {ks[1]} against {ks[0]}")
    assert ks[0] - ks[1] == sum(sizes) - len(sizes)
    assert rms[1] <= 2 * rms[0], f"{name}: lazy {rms[1]:.3e} against default {rms[0]:.3e} (bound 2 x)"
