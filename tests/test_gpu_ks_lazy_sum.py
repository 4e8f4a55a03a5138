"""GPU: lazy sums on SEAL-layout keys (dacapo_amd/csrc/hoist_ks.hip f_ks_gsum_kernel; option ks_lazy_sum, dc_ct_rotate_sum_hoisted) against
the oracle composition that tests/test_ks_lazy_sum_oracle.py checks -- per member orc_rotate_acc_hybrid at one special prime and one prime per
digit, Oracle.lazy_mul_plain / lazy_add, one orc_moddown_hybrid per sum -- limb for limb:
  * kernel level: one member (the hoisted hop), distinct and shared sources, bare and plaintext members and a mix, the destination on a source,
    20 members (more than one 16-product accumulator window in both forms), the reference's ring; every forced launch shape;
  * VM level: a two-layer convolution-shaped program under both option values and three execution modes equals the oracle VM that replays the
    exported groups; the groups are what the program implies; plan = 0, the option off, a small max_batch and two streams;
  * misuse is refused with a message, and the ResNet-20 inference with its taps in lazy sums still decrypts to the torch logits."""
import ctypes as C
import gc
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_helpers import _get_ct, _import_keys, _mirror_vm  # noqa: E402
from oracle.oracle import Ciphertext, Plaintext, splitmix_fill  # noqa: E402
from test_ks_lazy_sum_oracle import LazyOracle  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
STEPS = [1, -3, 2, 5, -1]


def _new_symbols():
    """the entry point and the option this feature adds (an AttributeError / a failed assertion where the library or the binding lacks them)"""
    from dacapo_amd import lowlevel as ll

    assert '"ks_lazy_sum"' in (ROOT / "dacapo_amd" / "csrc" / "options.cpp").read_text()
    return ll.lib().dc_ct_rotate_sum_hoisted


_RINGS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _release_rings_after_the_module():
    """contexts, key buffers and the entry point's scratch are shared by this module's tests and freed with it"""
    yield
    _RINGS.clear()
    gc.collect()


def _ring(logN, K):
    """oracle, keys of the five elements (host and device), a context and a cache of sources / plaintexts / expected sums, made once per ring"""
    from dacapo_amd import lowlevel as ll

    if (logN, K) not in _RINGS:
        o = LazyOracle(logN, K)
        elts = [o.elt_from_step(s) for s in STEPS]
        o.keygen(seed=0x4845564D, galois_elts=elts, relin=False)
        ctx = ll.Context(logN, K)
        assert ctx.primes == o.primes
        _RINGS[(logN, K)] = (o, elts, {e: ll.DeviceBuffer.from_host(o.galois[e]) for e in elts}, ctx, {})
    return _RINGS[(logN, K)]


def _source(ring, ell, which):
    o, cache = ring[0], ring[4]
    if ("src", ell, which) not in cache:
        q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
        cache[("src", ell, which)] = np.stack(
            [np.stack([splitmix_fill(1 + 7 * p + i + 100 * ell + 1000 * which, o.N) for i in range(ell)]) % q for p in range(2)])
    return cache[("src", ell, which)]


def _plain(ring, which):
    """plaintext `which` encoded at all K primes: [K][N]; the data limbs are [:l], the special-prime limb is [K-1:K]"""
    o, cache = ring[0], ring[4]
    if ("pt", which) not in cache:
        v = np.random.default_rng(1000 + which).uniform(-1, 1, o.slots)
        cache[("pt", which)] = np.ascontiguousarray(o.encode(v, 2.0**40, o.K).data)
    return cache[("pt", which)]


def _want(ring, ell, members):
    """the oracle's sum, computed once per (level, member list).  members: (source index, element, plaintext index or None)"""
    o, cache = ring[0], ring[4]
    key = ("sum", ell, tuple(members))
    if key not in cache:
        ms = []
        for si, elt, pi in members:
            pt = None if pi is None else Plaintext(np.ascontiguousarray(_plain(ring, pi)[:ell]), 2.0**40)
            sp = None if pi is None else np.ascontiguousarray(_plain(ring, pi)[o.K - 1 : o.K])
            ms.append((Ciphertext(_source(ring, ell, si), 2.0**40), elt, pt, sp))
        cache[key] = o.rotate_sum(ms, ell).data
    return cache[key]


def _rotate_sum(ring, ell, members, dst_on=None):
    """dc_ct_rotate_sum_hoisted of `members` -> (the sum, the sources read back afterwards by index).  dst_on: the source index the
    destination aliases, or None for a buffer of its own"""
    from dacapo_amd import lowlevel as ll

    fn = _new_symbols()
    o, _, dkeys, ctx, _ = ring
    n, N, K = len(members), o.N, o.K
    srcs = {si: ll.DeviceBuffer.from_host(_source(ring, ell, si)) for si, _, _ in members}
    pts = {pi: (ll.DeviceBuffer.from_host(_plain(ring, pi)[:ell]), ll.DeviceBuffer.from_host(_plain(ring, pi)[K - 1 : K]))
           for _, _, pi in members if pi is not None}
    out = srcs[dst_on] if dst_on is not None else ll.DeviceBuffer((2, ell, N))
    sp = (C.c_void_p * n)(*[srcs[si].ptr for si, _, _ in members])
    ge = (C.c_uint32 * n)(*[e for _, e, _ in members])
    keys = (C.c_void_p * n)(*[dkeys[e].ptr for _, e, _ in members])
    if pts:
        pl = (C.c_void_p * n)(*[pts[pi][0].ptr if pi is not None else None for _, _, pi in members])
        ps = (C.c_void_p * n)(*[pts[pi][1].ptr if pi is not None else None for _, _, pi in members])
    else:
        pl = ps = None
    fn(ctx.h, out.ptr, ell * N, sp, ell * N, ge, keys, pl, ps, n, ell, None)
    ll.lib().dc_stream_sync(None)
    return out.to_host(), {si: d.to_host() for si, d in srcs.items() if si != dst_on}


def _seven(ring):
    """five members of one source and two of another, all with plaintexts"""
    e = ring[1]
    return [(0, e[0], 0), (0, e[1], 1), (0, e[2], 2), (0, e[3], 3), (0, e[4], 4), (1, e[0], 5), (1, e[3], 6)]


@pytest.mark.parametrize("ell", [1, 3, 5])
def test_one_bare_member_is_the_hoisted_hop(ell):
    """count = 1 without a plaintext == dc_ct_rotate_hoisted == the oracle's hoisted hop (N = 2^12, K = 6)"""
    from dacapo_amd import lowlevel as ll

    ring = _ring(12, 6)
    o, elts, dkeys, ctx, _ = ring
    N = o.N
    for elt in elts[:3]:
        got, _ = _rotate_sum(ring, ell, [(0, elt, None)])
        assert (got == o.apply_galois(Ciphertext(_source(ring, ell, 0), 2.0**40), elt).data).all(), (ell, elt)
        assert (got == _want(ring, ell, [(0, elt, None)])).all(), (ell, elt)
        da, dd = ll.DeviceBuffer.from_host(_source(ring, ell, 0)), ll.DeviceBuffer((2, ell, N))
        ll.lib().dc_ct_rotate_hoisted(ctx.h, (C.c_void_p * 1)(dd.ptr), ell * N, da.ptr, ell * N, (C.c_uint32 * 1)(elt),
                                      (C.c_void_p * 1)(dkeys[elt].ptr), 1, ell, None)
        ll.lib().dc_stream_sync(None)
        assert (got == dd.to_host()).all(), (ell, elt)


@pytest.mark.parametrize("ell", [1, 3, 5])
def test_three_bare_members_of_distinct_sources(ell):
    ring = _ring(12, 6)
    e = ring[1]
    members = [(0, e[0], None), (1, e[1], None), (2, e[3], None)]
    got, after = _rotate_sum(ring, ell, members)
    assert (got == _want(ring, ell, members)).all()
    assert all((after[si] == _source(ring, ell, si)).all() for si in after)


def test_shared_sources_with_plaintexts_and_destination_on_a_source():
    """five members of one source + two of another, all times plaintexts, l = 3: the oracle's limbs, the sources unchanged; the same with the
    destination on either source (every read of a source precedes the only launch that writes a destination)"""
    ring = _ring(12, 6)
    members = _seven(ring)
    got, after = _rotate_sum(ring, 3, members)
    assert (got == _want(ring, 3, members)).all()
    assert all((after[si] == _source(ring, 3, si)).all() for si in (0, 1))
    for on in (0, 1):
        got, after = _rotate_sum(ring, 3, members, dst_on=on)
        assert (got == _want(ring, 3, members)).all(), on
        assert (after[1 - on] == _source(ring, 3, 1 - on)).all()


def test_mixed_bare_and_plaintext_members():
    ring = _ring(12, 6)
    e = ring[1]
    members = [(0, e[0], 0), (0, e[1], None), (1, e[2], 1), (2, e[3], None), (1, e[4], None), (2, e[0], 2)]
    got, _ = _rotate_sum(ring, 3, members)
    assert (got == _want(ring, 3, members)).all()


@pytest.mark.parametrize("plain", [False, True])
def test_twenty_members_cross_the_accumulator_fold(plain):
    """l = 2: 20 bare members put 20 * (2 products + a base term) through one accumulator pair, 20 plaintext members 20 products -- both more
    than the 16 an Acc128 holds between folds; elements repeat"""
    ring = _ring(12, 6)
    e = ring[1]
    members = [(k % 3, e[(k * 2) % 5], (k % 7) if plain else None) for k in range(20)]
    got, _ = _rotate_sum(ring, 2, members)
    assert (got == _want(ring, 2, members)).all()


def test_reference_ring_three_members_with_plaintexts():
    """N = 2^15, K = 14, l = 13: the reference's ring and top level (a member's own accumulators take 14 products), the large-batch lift"""
    ring = _ring(15, 14)
    e = ring[1]
    members = [(0, e[0], 0), (0, e[1], 1), (1, e[3], 2)]
    got, after = _rotate_sum(ring, 13, members)
    assert (got == _want(ring, 13, members)).all()
    assert all((after[si] == _source(ring, 13, si)).all() for si in after)


@pytest.mark.parametrize("opts", [dict(tiny_tile_wgs=0, small_tile_wgs=0), dict(tiny_tile_wgs=0, small_tile_wgs=1 << 30), dict(tiny_tile_wgs=100000),
                                  dict(ks_merge_special_min_wgs=0), dict(ks_merge_special_min_wgs=0, tiny_tile_wgs=0),
                                  dict(ks_items_fast=0), dict(ks_items_fast=1),
                                  dict(tiny_tile_wgs=0, small_tile_wgs=0, wide_tile_wgs=0, ks_big_tiles=0), dict(wide_tile_wgs=-1, ks_big_tiles=0),
                                  dict(ks_big_tiles=0, ks_merge_lift_min_wgs=0), dict(tiny_tile_wgs=0, ks_merge_lift_min_wgs=0)])
def test_sums_under_every_forced_launch_shape(opts):
    """N = 2^12, l = 3, a group of one and a group of seven: the option sets of tests/test_gpu_ks_hoist.py that reach this kernel and its tail"""
    from dacapo_amd import runner

    ring = _ring(12, 6)
    one, seven = [(0, ring[1][1], None)], _seven(ring)
    with runner.options(**opts):
        got1, _ = _rotate_sum(ring, 3, one)
        got7, _ = _rotate_sum(ring, 3, seven)
    assert (got1 == _want(ring, 3, one)).all(), opts
    assert (got7 == _want(ring, 3, seven)).all(), opts


TAPS = ((0, (1, 2, 3, 5, -1)), (1, (1, 4)))   # per layer: (input, offsets) times plaintexts
BARE = ((0, 1), (0, 2), (1, 3))               # per layer: the bare part rot(u, 1) + rot(u, 2) + rot(v, 3)
LAYERS = 2


def _two_layer_program(slots, levels):
    """two layers of: taps of two inputs times plaintexts (3 and 5 are two-hop NAF offsets under the default keys) plus a bare part
    rot(u, 1) + rot(u, 2) + rot(v, 3) -- a sum of its own, which then enters the layer's sum times a plaintext (a bare rotation sits at the
    waterline and cannot meet the products' scale inside one sum) -- and a rescale between the layers"""
    from dacapo_amd import hevm_asm as ha

    rng = np.random.default_rng(17)
    b = ha.Builder(slots=slots, init_level=levels, policy="lazy", boot_level=levels, shadow=True)
    x, y = b.input(rng.uniform(-1, 1, slots)), b.input(rng.uniform(-1, 1, slots))

    def layer(u, v):
        ins, acc = (u, v), None
        for which, offs in TAPS:
            for k in offs:
                t = b.mul_plain(b.rotate(ins[which], k), rng.uniform(-0.5, 0.5, slots))
                acc = t if acc is None else b.add(acc, t)
        s = None
        for which, k in BARE:
            r = b.rotate(ins[which], k)
            s = r if s is None else b.add(s, r)
        return b.rescale(b.add(acc, b.mul_plain(s, rng.uniform(-0.5, 0.5, slots))))

    r = layer(x, y)
    r2 = b.rescale(b.mul_plain(y, rng.uniform(-0.5, 0.5, slots)))
    assert LAYERS == 2
    out = layer(r, r2)
    # A value that still sits in a register when the program ends can be read by the host, so the plan keeps it as it is ("pinned": never a
    # member).  The assembler recycles dead registers, and without more work after the second layer its last rotations would stay in theirs.
    # Four products alive at once take every register the layers used; what stays behind then is these products and their sums.
    tail = [b.mul_plain(out, rng.uniform(-0.5, 0.5, slots)) for _ in range(4)]
    b.output(b.finish(b.add(b.add(tail[0], tail[1]), b.add(tail[2], tail[3]))))
    return b


def _layer_values_left_in_registers(hv_ops):
    """instruction indices up to the program's last rotation whose destination register is never written again: rotations and the partial sums
    between them (ops: (opcode, dst, lhs, rhs); opcode 0 / 16 write plaintext registers)"""
    ct = [(i, op) for i, op in enumerate(hv_ops) if op[0] not in (0, 16, 0xFFFF)]
    last_rot = max(i for i, op in ct if op[0] == 1)
    return [i for k, (i, op) in enumerate(ct) if i <= last_rot and all(o[1] != op[1] for _, o in ct[k + 1:])]


def _expected_groups(lazy):
    """group sizes the program implies: per layer the bare part (every value), and under 2 the layer's taps"""
    taps = sum(len(offs) for _, offs in TAPS)
    return sorted(([len(BARE)] + ([taps] if lazy == 2 else [])) * LAYERS) if lazy else []


def _expected_hops(o):
    return LAYERS * (sum(len(o.rotate_hops(k)) for _, offs in TAPS for k in offs) + sum(len(o.rotate_hops(k)) for _, k in BARE))


def _run_vm_program(tmp_path, lazy, plan=1, graph=1, streams=1, extra=None):
    """run the program on a VM with ks_hoist = 1, ks_lazy_sum = lazy; compare every stream's result with the oracle VM replaying the exported
    groups -> (groups, hoist stats)"""
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    _new_symbols()
    logN, K = 12, 6
    opts = {"plan": plan, "plan_graph": graph, "ks_hoist": 1, "ks_lazy_sum": lazy}
    opts.update(extra or {})
    hevm = runner.HEVM(seed=77, logN=logN, num_primes=K, vm_options=opts)
    if streams > 1:
        hevm.set_streams(streams)
    o = LazyOracle(logN, K)
    _import_keys(o, hevm, ll)
    b = _two_layer_program(1 << (logN - 1), K - 1)
    cst, hv, _ = b.assemble()
    hevm.load_mem(cst, hv)
    ovm0 = _mirror_vm(hevm, ll, o, cst, hv, tmp_path)
    # (what _expected_groups assumes: no value of the two layers is still in a register at the end, where the plan would have to keep it)
    assert _layer_values_left_in_registers([tuple(int(v) for v in op) for op in ovm0.prog.ops]) == []
    for q in range(streams):
        if streams > 1:
            hevm.select_stream(q)
        for i, a in enumerate(b.args):
            hevm.setInput(i, a.plain if q == 0 else a.plain[::-1].copy())
    hevm.run()
    groups = hevm.lazy_groups()
    for q in range(streams):
        if streams > 1:
            hevm.select_stream(q)
        ovm = _mirror_vm(hevm, ll, o, cst, hv, tmp_path)
        ovm.plains_special = {}
        for i in range(ovm.prog.num_ptxt):  # the special-prime limbs the plan encoded for its members' plaintexts: [1][N]
            p = hevm.lw.hevm_plain_special(hevm.vm, i)
            if p:
                ovm.plains_special[i] = ll.read_device(p, (1, o.N))
        if groups:
            ovm.set_lazy_groups(groups)
        for i in range(len(b.args)):  # (program inputs live in their home buffers, which the plan never overwrites)
            ovm.ciphers[i] = _get_ct(hevm, ll, i)
        ovm.run()
        r = ovm.prog.res_dst[0]
        got, want = _get_ct(hevm, ll, r), ovm.ciphers[r]
        assert got.ell == want.ell and got.scale == want.scale
        assert (got.data == want.data).all(), (lazy, plan, graph, q)
        if q == 0:
            assert np.abs(hevm.getOutput()[0] - b.expected()[0]).max() < 1e-5
        n_special = len(ovm.plains_special)
    st = hevm.hoist_stats()
    hevm.close()
    assert st["hops"] == streams * _expected_hops(o)
    return groups, st, n_special


@pytest.mark.parametrize("lazy", [1, 2])
@pytest.mark.parametrize("plan,graph", [(1, 1), (1, 0), (1, 2)])
def test_vm_program_equals_the_oracle_vm_replaying_the_groups(tmp_path, plan, graph, lazy):
    """the result's limbs, level and scale equal the oracle VM's under the exported groups; the groups are exactly what the program implies
    (1: the bare parts; 2: the taps too, whose plaintexts -- and only those -- get a special-prime limb); every hop is still counted"""
    groups, st, n_special = _run_vm_program(tmp_path, lazy, plan, graph)
    print(plan, graph, lazy, [len(g) for g in groups], st, n_special)
    assert sorted(len(g) for g in groups) == _expected_groups(lazy), groups
    assert n_special == (LAYERS * sum(len(offs) for _, offs in TAPS) if lazy == 2 else 0)


@pytest.mark.parametrize("lazy", [1, 2])
def test_the_loop_runs_every_rotation_on_its_own_hop(tmp_path, lazy):
    """plan = 0: no groups (hevm_plan_lazy_groups returns -1), the hoisted oracle VM's limbs"""
    groups, st, _ = _run_vm_program(tmp_path, lazy, plan=0, graph=1)
    assert groups == []
    assert st["decompositions"] == st["hops"]


def test_option_off_changes_nothing(tmp_path):
    """ks_lazy_sum = 0 (ks_hoist = 1): no groups, the hoisted oracle VM's limbs"""
    groups, st, n_special = _run_vm_program(tmp_path, 0)
    assert groups == [] and n_special == 0


def test_small_max_batch_keeps_whole_groups(tmp_path):
    """max_batch = 4, value 2: docs/design/kernels.md -- a group is never split and never shrinks with max_batch; a step holds whole groups up
    to max_batch members or ONE larger group, and the scratch is sized for the largest step.  Still the oracle's limbs under the exported groups."""
    groups, _, _ = _run_vm_program(tmp_path, 2, extra={"max_batch": 4})
    assert sorted(len(g) for g in groups) == _expected_groups(2), groups


def test_two_streams_each_equal_their_own_oracle_run(tmp_path):
    groups, st, _ = _run_vm_program(tmp_path, 2, plan=1, graph=0, streams=2)
    assert sorted(len(g) for g in groups) == _expected_groups(2), groups


def _child(code):
    return subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), capture_output=True, text=True, timeout=120)


def test_ks_lazy_sum_needs_ks_hoist():
    _new_symbols()
    r = _child("from dacapo_amd import runner\n"
               "runner.HEVM(fresh=True, logN=12, num_primes=6, vm_options={'ks_lazy_sum': 1, 'ks_hoist': 0})\n"
               "print('created')\n")
    assert r.returncode != 0 and "created" not in r.stdout, (r.returncode, r.stdout)
    assert "ks_lazy_sum" in r.stderr and "ks_hoist" in r.stderr, r.stderr


def test_ks_lazy_sum_is_refused_with_grouped_digits():
    _new_symbols()
    r = _child("from dacapo_amd import runner\n"
               "runner.HEVM(fresh=True, logN=12, num_primes=6, ks_special=2, vm_options={'ks_lazy_sum': 1})\n"
               "print('created')\n")
    assert r.returncode != 0 and "created" not in r.stdout, (r.returncode, r.stdout)
    assert "ks_lazy_sum" in r.stderr and "ks_special = 2" in r.stderr and "hyb_lazy_sum" in r.stderr, r.stderr


def test_rotate_sum_entry_is_refused_on_a_grouped_digit_context():
    _new_symbols()
    r = _child("import ctypes as C\n"
               "from dacapo_amd import lowlevel as ll\n"
               "ctx = ll.Context(12, 6, special=2)\n"
               "N = 1 << 12\n"
               "a, d, k = ll.DeviceBuffer((2, 2, N)), ll.DeviceBuffer((2, 2, N)), ll.DeviceBuffer((2, 2, 6, N))\n"
               "ll.lib().dc_ct_rotate_sum_hoisted(ctx.h, d.ptr, 2 * N, (C.c_void_p * 1)(a.ptr), 2 * N, (C.c_uint32 * 1)(3), (C.c_void_p * 1)(k.ptr),\n"
               "                                  None, None, 1, 2, None)\n"
               "print('created')\n")
    assert r.returncode != 0 and "created" not in r.stdout, (r.returncode, r.stdout)
    assert "dc_ct_rotate_sum_hoisted" in r.stderr and "grouped digits" in r.stderr, r.stderr


def test_resnet20_with_lazy_sums_matches_torch():
    """the headline fixture with ks_hoist = 1, ks_lazy_sum = 2: argmax and rms < 3e-3 against torch (the bound tests/test_gpu_resnet20.py applies
    to the default run); the static count of the fixture gives 25 sums of 707 taps (plus four sums of two)"""
    _new_symbols()
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
    hevm = runner.HEVM(seed=0x4845564D, logN=15, num_primes=14, vm_options={"ks_hoist": 1, "ks_lazy_sum": 2})
    hevm.load_mem(fx["cst"], fx["hevm"])
    hevm.setInput(0, fx["packed"])
    hevm.run()
    out = hevm.getOutput()[0]
    logits, want = out[:10] * 32, fx["torch_result"]
    rms_torch = float(np.sqrt(np.mean((logits - want) ** 2)))
    groups = hevm.lazy_groups()
    members = sum(len(g) for g in groups)
    print(f"ResNet-20 with ks_lazy_sum = 2: {len(groups)} groups, {members} rotations in groups, rms vs torch {rms_torch:.3e}")
    assert int(np.argmax(logits)) == int(np.argmax(want))
    assert rms_torch < 3e-3
    assert len(groups) >= 20 and members > 600
    hevm.close()
