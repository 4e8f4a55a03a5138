"""GPU: flattened rotate-and-add chains (option ks_flatten_sums; dacapo_amd/csrc/plan_flatten.cpp, hoist_ks.hip f_ks_gsum_kernel with an addend,
dc_ct_rotate_sum_hoisted_add) against the oracle composition Oracle.add(addend, LazyOracle.rotate_sum(members, l)), limb for limb.  N = 2^12, K = 4.
  * entry point at l = 1, 2, 3: one source with 1, 3, 7, 15, 16 and 63 members plus an addend (15 / 16: either side of the accumulator's
    16-product window at l = 1, where a member brings a base term and one digit; every other count crosses it somewhere); the addend a
    third ciphertext, a source, the destination, NULL (== dc_ct_rotate_sum_hoisted); two sources; every forced launch shape;
  * VM: a program of chains of 2, 3, 5 and 6 hops and near-misses (a third reader, an interior result, a rotation read twice, either operand
    order, a subset sum of 0) with the composite keys added through flatten_offsets() -> addRotationKeys, f = 2, 3, 6, three execution modes,
    one and two streams: every result limb == an oracle VM that replays exactly the exported groups with the oracle's own arithmetic; the
    exported groups are what the restatement of the rules in tests/test_plan_flatten.py implies; one composite key withheld; option 0;
  * the decrypted error stays within 2x the option-off run's, and the headline program at f = 3 keeps the torch logits."""
import ctypes as C
import gc
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_helpers import _get_ct, _import_keys, _mirror_vm  # noqa: E402
from oracle.oracle import Ciphertext, splitmix_fill  # noqa: E402
from test_ks_lazy_sum_oracle import LazyOracle  # noqa: E402
from test_plan_flatten import flatten_groups, totals  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
LOGN, K = 12, 4
HOPS = [1, 2, 4, 8, 16, 32]  # a six-hop stage: the 63 subset sums are the offsets 1 .. 63


def _entry():
    """the entry point and the option this feature adds (an AttributeError / a failed assertion where the library or the binding lacks them)"""
    from dacapo_amd import lowlevel as ll

    assert '"ks_flatten_sums"' in (ROOT / "dacapo_amd" / "csrc" / "options.cpp").read_text()
    return ll.lib().dc_ct_rotate_sum_hoisted_add


_RING: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_ring_after_the_module():
    yield
    _RING.clear()
    gc.collect()


def _ring():
    """oracle, the elements of the offsets 1 .. 63, their keys (host and device), a context and a cache of sources / expected sums, made once"""
    from dacapo_amd import lowlevel as ll

    if not _RING:
        o = LazyOracle(LOGN, K)
        elts = [o.elt_from_step(s) for s in range(1, 64)]
        o.keygen(seed=0x4845564D, galois_elts=elts, relin=False)
        ctx = ll.Context(LOGN, K)
        assert ctx.primes == o.primes
        _RING["r"] = (o, elts, {e: ll.DeviceBuffer.from_host(o.galois[e]) for e in elts}, ctx, {})
    return _RING["r"]


def _source(ring, ell, which):
    o, cache = ring[0], ring[4]
    if ("src", ell, which) not in cache:
        q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
        cache[("src", ell, which)] = np.stack(
            [np.stack([splitmix_fill(3 + 7 * p + i + 100 * ell + 1000 * which, o.N) for i in range(ell)]) % q for p in range(2)])
    return cache[("src", ell, which)]


def _sum(ring, ell, members):
    """LazyOracle.rotate_sum of the bare members (source index, element), computed once per (level, member list)"""
    o, cache = ring[0], ring[4]
    key = ("sum", ell, tuple(members))
    if key not in cache:
        cache[key] = o.rotate_sum([(Ciphertext(_source(ring, ell, si), 2.0**40), elt, None, None) for si, elt in members], ell)
    return cache[key]


def _want(ring, ell, members, addend):
    """Oracle.add(addend, the lazy sum); addend: a source index or None"""
    o = ring[0]
    s = _sum(ring, ell, members)
    return s.data if addend is None else o.add(Ciphertext(_source(ring, ell, addend), 2.0**40), s).data


def _rotate_sum_add(ring, ell, members, addend, dst_on=None, entry="add"):
    """dc_ct_rotate_sum_hoisted_add (or, entry = "plain", dc_ct_rotate_sum_hoisted) -> (the result, the other buffers read back afterwards).
    addend / dst_on: the index of the source whose buffer is the addend / the destination (an index no member names: a ciphertext of its own)"""
    from dacapo_amd import lowlevel as ll

    _entry()
    o, _, dkeys, ctx, _ = ring
    N = o.N
    used = {si for si, _ in members} | ({addend} if addend is not None else set()) | ({dst_on} if dst_on is not None else set())
    bufs = {si: ll.DeviceBuffer.from_host(_source(ring, ell, si)) for si in used}
    out = bufs[dst_on] if dst_on is not None else ll.DeviceBuffer((2, ell, N))
    srcs, elts, keys = [bufs[si].ptr for si, _ in members], [e for _, e in members], [dkeys[e].ptr for _, e in members]
    if entry == "add":
        ctx.rotate_sum_add(out.ptr, ell * N, bufs[addend].ptr if addend is not None else None, ell * N, srcs, ell * N, elts, keys, ell)
    else:
        n = len(members)
        ll.lib().dc_ct_rotate_sum_hoisted(ctx.h, out.ptr, ell * N, (C.c_void_p * n)(*srcs), ell * N, (C.c_uint32 * n)(*elts), (C.c_void_p * n)(*keys),
                                          None, None, n, ell, None)
    ll.lib().dc_stream_sync(None)
    return out.to_host(), {si: d.to_host() for si, d in bufs.items() if si != dst_on}


def _stage(ring, hops):
    """the members of a flattened stage of `hops` hops of source 0: the subset sums of HOPS[:hops], in the pass's order"""
    elts = ring[1]
    return [(0, elts[sum(o for k, o in enumerate(HOPS[:hops]) if mask >> k & 1) - 1]) for mask in range(1, 1 << hops)]


@pytest.mark.parametrize("ell", [1, 2, 3])
@pytest.mark.parametrize("count", [1, 3, 7, 15, 16, 63])
def test_one_source_plus_an_addend(ell, count):
    """1, 3, 7, 63: stages of 1, 2, 3 and 6 hops; 15 and 16 members: at l = 1 the addend and 15 members' base terms and digits are 31 products,
    one fold; with 16 members a second fold falls on the last digit"""
    ring = _ring()
    members = _stage(ring, 6)[:count]
    got, after = _rotate_sum_add(ring, ell, members, addend=5)
    assert (got == _want(ring, ell, members, 5)).all()
    assert all((after[si] == _source(ring, ell, si)).all() for si in after)


@pytest.mark.parametrize("ell", [1, 2, 3])
def test_the_addend_may_be_the_source_the_destination_or_null(ell):
    """seven members of source 0 (a three-hop stage): addend = the source (what a flattened stage passes), = dst, = a third ciphertext with
    dst on the source, and NULL, which is dc_ct_rotate_sum_hoisted itself"""
    ring = _ring()
    members = _stage(ring, 3)
    got, after = _rotate_sum_add(ring, ell, members, addend=0)
    assert (got == _want(ring, ell, members, 0)).all() and (after[0] == _source(ring, ell, 0)).all()
    got, after = _rotate_sum_add(ring, ell, members, addend=5, dst_on=5)
    assert (got == _want(ring, ell, members, 5)).all() and (after[0] == _source(ring, ell, 0)).all()
    got, after = _rotate_sum_add(ring, ell, members, addend=0, dst_on=0)
    assert (got == _want(ring, ell, members, 0)).all()
    got, after = _rotate_sum_add(ring, ell, members, addend=5, dst_on=0)
    assert (got == _want(ring, ell, members, 5)).all() and (after[5] == _source(ring, ell, 5)).all()
    got, _ = _rotate_sum_add(ring, ell, members, addend=None)
    plain, _ = _rotate_sum_add(ring, ell, members, addend=None, entry="plain")
    assert (got == plain).all() and (got == _want(ring, ell, members, None)).all()


@pytest.mark.parametrize("ell", [1, 2, 3])
def test_two_sources_plus_an_addend(ell):
    ring = _ring()
    e = ring[1]
    members = [(0, e[0]), (1, e[1]), (0, e[2]), (1, e[4]), (1, e[0])]
    for addend in (1, 7):
        got, after = _rotate_sum_add(ring, ell, members, addend=addend)
        assert (got == _want(ring, ell, members, addend)).all(), addend
        assert all((after[si] == _source(ring, ell, si)).all() for si in after)


@pytest.mark.parametrize("opts", [dict(tiny_tile_wgs=0, small_tile_wgs=0), dict(tiny_tile_wgs=0, small_tile_wgs=1 << 30), dict(tiny_tile_wgs=100000),
                                  dict(ks_merge_special_min_wgs=0), dict(ks_merge_special_min_wgs=0, tiny_tile_wgs=0),
                                  dict(ks_items_fast=0), dict(ks_items_fast=1),
                                  dict(tiny_tile_wgs=0, small_tile_wgs=0, wide_tile_wgs=0, ks_big_tiles=0), dict(wide_tile_wgs=-1, ks_big_tiles=0),
                                  dict(ks_big_tiles=0, ks_merge_lift_min_wgs=0), dict(tiny_tile_wgs=0, ks_merge_lift_min_wgs=0)])
def test_an_addend_under_every_forced_launch_shape(opts):
    """l = 3, a group of one and a group of seven, each plus an addend: the option sets tests/test_gpu_ks_lazy_sum.py forces"""
    from dacapo_amd import runner

    ring = _ring()
    one, seven = _stage(ring, 1), _stage(ring, 3)
    with runner.options(**opts):
        got1, _ = _rotate_sum_add(ring, 3, one, addend=0)
        got7, _ = _rotate_sum_add(ring, 3, seven, addend=5)
    assert (got1 == _want(ring, 3, one, 0)).all(), opts
    assert (got7 == _want(ring, 3, seven, 5)).all(), opts


# ---- VM level (option ks_flatten_sums) -------------------------------------------------------------------------------------------------------
def _chain_program(slots, levels):
    """chains of 6, 5, 3 and 2 hops and the near-misses, every chain's end feeding the one result:
      A  six hops of x by 1 .. 32;                      B  five hops of y by 3, 6, 12, 24, 48 (no direct keys), the rotation first in every add;
      C  three hops of A's end + x (a value of its own, so that A ends where it ends) whose first interior value has a third reader (cut
         after the first hop);
      D  two hops by slots / 2 each (their sum is 0: left as written);
      E  two hops of B's end whose first rotation is read twice (no hop; the second hop is a chain of one);
      F  four hops of B's end whose second interior value is a result (cut in the middle);     G  two hops of x by -1 and 5;
      H  three hops of y by 9, 18, 36;      I  two hops by 11 and 22 of x + y, a sum that nothing but the stage reads"""
    from dacapo_amd import hevm_asm as ha

    rng = np.random.default_rng(23)
    b = ha.Builder(slots=slots, init_level=levels, policy="lazy", boot_level=levels, shadow=True)
    x, y = b.input(rng.uniform(-1e-3, 1e-3, slots)), b.input(rng.uniform(-1e-3, 1e-3, slots))

    def hops(v, offsets, rot_first=False, keep=None):
        for k, o in enumerate(offsets):
            r = b.rotate(v, o)
            v = b.add(r, v) if rot_first else b.add(v, r)
            if keep is not None:
                keep.append(v)
        return v

    a_end = hops(x, [1, 2, 4, 8, 16, 32])
    b_end = hops(y, [3, 6, 12, 24, 48], rot_first=True)
    c_vals = []
    c_end = hops(b.add(a_end, x), [64, 128, 256], keep=c_vals)
    c_end = b.add(c_end, c_vals[0])
    d_end = hops(x, [slots // 2, slots // 2])
    r = b.rotate(b_end, 5)
    e_end = b.add(hops(b.add(b_end, r), [10]), r)
    f_vals = []
    f_end = hops(b_end, [7, 14, 28, 56], keep=f_vals)
    g_end = hops(x, [-1, 5])
    h_end = hops(y, [9, 18, 36])
    i_end = hops(b.add(x, y), [11, 22])
    total = c_end
    for v in (d_end, e_end, f_end, g_end, h_end, i_end):
        total = b.add(total, v)
    b.output(b.finish(total))
    b.output(b.finish(f_vals[1]))
    return b


class _ReplayVM:
    """the oracle VM with the exported groups applied: a stage's rotations and its adds but the closing one do nothing, the closing add writes
    Oracle.add(source, LazyOracle.rotate_sum(the members of the source)) -- the source is what the stage's first rotation read"""

    def __init__(self, ovm, groups):
        self.ovm, self.closing, self.first_rot, self.skip, self.source = ovm, {}, {}, set(), {}
        for g, (closing, pairs, offsets) in enumerate(groups):
            self.closing[closing] = (g, offsets)
            self.first_rot[pairs[0][0]] = g
            self.skip |= {i for pair in pairs for i in pair} - {closing}

    def run(self):
        ovm, o = self.ovm, self.ovm.o
        for index, op in enumerate(ovm.prog.ops):
            opcode, dst, lhs, rhs = (int(v) for v in op)
            if index in self.first_rot:
                self.source[self.first_rot[index]] = ovm.ciphers[lhs]
            if index in self.closing:
                g, offsets = self.closing[index]
                src = self.source[g]
                s = o.rotate_sum([(src, o.elt_from_step(off), None, None) for off in offsets], src.ell)
                ovm.ciphers[dst] = o.add(src, s)
            elif index not in self.skip:
                ovm.step(op, index)


def _expected_groups(hv, f, slots, keyed=None):
    from dacapo_amd import hevm_asm as ha

    prog = ha.unpack_hevm(hv)
    return [(c, pairs, members) for c, _, pairs, members in flatten_groups(prog["ops"], prog["res_dst"], f, slots, keyed)]


def _run_chain_program(tmp_path, f, graph=1, streams=1, withhold=0, plan=1):
    """the program under ks_hoist = 1, ks_lazy_sum = 1, ks_flatten_sums = f with the composite keys added (all but the last `withhold`): every
    result register of every stream == the replay of the exported groups -> (exported groups, stats, offsets added, decrypted error)"""
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    _entry()
    slots = 1 << (LOGN - 1)
    opts = {"plan": plan, "plan_graph": graph, "ks_hoist": 1, "ks_lazy_sum": 1, "ks_flatten_sums": f}
    hevm = runner.HEVM(seed=93, logN=LOGN, num_primes=K, vm_options=opts)
    if streams > 1:
        hevm.set_streams(streams)
    b = _chain_program(slots, K - 1)
    cst, hv, _ = b.assemble()
    hevm.load_mem(cst, hv)
    o = LazyOracle(LOGN, K)
    missing = hevm.flatten_offsets()
    if f and plan:
        want_all = {off for _, _, members in _expected_groups(hv, f, slots) for off in members}
        assert missing == sorted(off for off in want_all if o.elt_from_step(off) not in o.default_galois_elts())
    else:
        assert missing == []
    added = missing[: len(missing) - withhold]
    if added:
        hevm.addRotationKeys(added)
        assert hevm.flatten_offsets() == missing[len(missing) - withhold :]
    _import_keys(o, hevm, ll, elts=o.default_galois_elts() + [o.elt_from_step(off) for off in added])
    for q in range(streams):
        if streams > 1:
            hevm.select_stream(q)
        for i, a in enumerate(b.args):
            hevm.setInput(i, a.plain if q == 0 else a.plain[::-1].copy())
    hevm.run()
    groups = hevm.flatten_groups()
    assert hevm.lazy_groups() == []  # (a hop has one rotation and one bare addend: no lazy sum of the existing pass)
    err = 0.0
    for q in range(streams):
        if streams > 1:
            hevm.select_stream(q)
        ovm = _mirror_vm(hevm, ll, o, cst, hv, tmp_path)
        for i in range(len(b.args)):
            ovm.ciphers[i] = _get_ct(hevm, ll, i)
        _ReplayVM(ovm, groups if isinstance(groups, list) else []).run()
        for r in ovm.prog.res_dst:
            got, want = _get_ct(hevm, ll, r), ovm.ciphers[r]
            assert got.ell == want.ell and got.scale == want.scale
            assert (got.data == want.data).all(), (f, graph, q, r)
        if q == 0:
            err = max(float(np.abs(got - ref).max()) for got, ref in zip(hevm.getOutput(), b.expected()))
    st = dict(hevm.flatten_stats(), keyswitches=hevm.stats()["keyswitches"]) if plan else hevm.flatten_stats()
    hevm.close()
    keyed = {(1 << k) * sg for k in range(LOGN - 1) for sg in (1, -1)} | set(added)  # (the default key set: +-2^k)
    if f and plan:
        assert groups == _expected_groups(hv, f, slots, keyed)
        n, hops, members, _, _ = totals([(g[0], 0, g[1], g[2]) for g in groups])
        assert st["groups"] == streams * n and st["hops_absorbed"] == streams * hops and st["members"] == streams * members
    return groups, st, added, err


@pytest.mark.parametrize("graph", [0, 1, 2])
@pytest.mark.parametrize("f", [2, 3, 6])
def test_chain_program_equals_the_replay_of_the_exported_groups(tmp_path, f, graph):
    groups, st, added, _ = _run_chain_program(tmp_path, f, graph)
    sizes = sorted(len(g[1]) for g in groups)
    print(f, graph, sizes, st, len(added))
    # A 6, B 5, C 1 + 2, D none, E none, F 2 + 2, G 2, H 3, I 2 hops: at f = 6 whole, below that split into stages of at most f
    assert sizes == {2: [2] * 11, 3: [2, 2, 2, 2, 2, 2, 3, 3, 3, 3], 6: [2, 2, 2, 2, 2, 3, 5, 6]}[f]


def test_two_streams_each_equal_their_own_replay(tmp_path):
    groups, st, _, _ = _run_chain_program(tmp_path, 3, graph=1, streams=2)
    assert len(groups) == 10 and st["groups"] == 20


def test_a_withheld_composite_key_leaves_its_stage_as_written(tmp_path):
    """without the largest composite offset (C's 128 + 256 at f = 2) that stage runs as the program's two hops: one group fewer, same replay"""
    full, _, added_all, _ = _run_chain_program(tmp_path, 2)
    groups, _, added, _ = _run_chain_program(tmp_path, 2, withhold=1)
    assert len(added) == len(added_all) - 1 and len(groups) == len(full) - 1
    assert all(added_all[-1] not in g[2] for g in groups)


def test_option_off_and_the_loop_change_nothing(tmp_path):
    """ks_flatten_sums = 0: no groups, no offsets asked for, the limbs of the hoisted oracle VM (a VM that never heard of the option); plan = 0
    ignores the option"""
    groups, st, added, _ = _run_chain_program(tmp_path, 0)
    assert groups == 0 and added == [] and st["groups"] == 0
    groups, st, added, _ = _run_chain_program(tmp_path, 3, plan=0)
    assert groups == -1 and st["groups"] == 0


def test_decrypted_error_stays_within_twice_the_unflattened_runs(tmp_path):
    """against the cleartext evaluation: one rounding per stage instead of one per hop (the margin of tests/test_gpu_lazy_relin.py)"""
    _, _, _, off = _run_chain_program(tmp_path, 0)
    for f in (3, 6):
        _, _, _, on = _run_chain_program(tmp_path, f)
        print(f"ks_flatten_sums {f}: max error vs cleartext {on:.3e}, off {off:.3e}")
        assert on <= 2 * off


def _child(code):
    return subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("opts,words", [({"ks_flatten_sums": 3}, ["ks_hoist = 1", "ks_lazy_sum >= 1"]),
                                        ({"ks_flatten_sums": 3, "ks_hoist": 1}, ["ks_lazy_sum >= 1"]),
                                        ({"ks_flatten_sums": 7, "ks_hoist": 1, "ks_lazy_sum": 1}, ["2 .. 6"])])
def test_ks_flatten_sums_names_what_is_missing(opts, words):
    _entry()
    r = _child("from dacapo_amd import runner\n"
               f"runner.HEVM(fresh=True, logN=12, num_primes=4, vm_options={opts!r})\n"
               "print('created')\n")
    assert r.returncode != 0 and "created" not in r.stdout, (r.returncode, r.stdout)
    assert "ks_flatten_sums" in r.stderr and all(w in r.stderr for w in words), r.stderr
    if "ks_hoist" in opts and opts["ks_flatten_sums"] == 3:
        assert "ks_hoist = 1" not in r.stderr, r.stderr


def test_ks_flatten_sums_is_refused_with_grouped_digits():
    _entry()
    r = _child("from dacapo_amd import runner\n"
               "runner.HEVM(fresh=True, logN=12, num_primes=6, ks_special=2, vm_options={'ks_flatten_sums': 3})\n"
               "print('created')\n")
    assert r.returncode != 0 and "created" not in r.stdout, (r.returncode, r.stdout)
    assert "ks_flatten_sums" in r.stderr and "ks_special = 2" in r.stderr, r.stderr


def test_resnet20_with_flattened_sums_matches_torch():
    """the headline fixture with ks_hoist = 1, ks_lazy_sum = 2, ks_flatten_sums = 3: argmax and rms < 3e-3 against torch (the bound of
    test_resnet20_with_lazy_sums_matches_torch); the run's counts are the pass's (tests/test_plan_flatten.py HEADLINE)"""
    _entry()
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
    hevm = runner.HEVM(seed=0x4845564D, logN=15, num_primes=14, vm_options={"ks_hoist": 1, "ks_lazy_sum": 2, "ks_flatten_sums": 3})
    hevm.load_mem(fx["cst"], fx["hevm"])
    missing = hevm.flatten_offsets()
    hevm.addRotationKeys(missing)
    assert hevm.flatten_offsets() == []
    hevm.setInput(0, fx["packed"])
    hevm.run()
    logits, want = hevm.getOutput()[0][:10] * 32, fx["torch_result"]
    rms_torch = float(np.sqrt(np.mean((logits - want) ** 2)))
    st, groups = hevm.flatten_stats(), hevm.flatten_groups()
    print(f"ResNet-20 with ks_flatten_sums = 3: {st}, {len(missing)} keys added, rms vs torch {rms_torch:.3e}")
    assert int(np.argmax(logits)) == int(np.argmax(want))
    assert rms_torch < 3e-3
    prog = ha.unpack_hevm(fx["hevm"])
    expected = flatten_groups(prog["ops"], prog["res_dst"], 3, 1 << 14)
    assert groups == [(c, pairs, members) for c, _, pairs, members in expected]
    n, hops, members, _, _ = totals(expected)
    assert (n, hops, members) == (648, 1569, 3036) and st == {"groups": n, "members": members, "hops_absorbed": hops}
    hevm.close()
