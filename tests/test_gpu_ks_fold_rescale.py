"""GPU: a rescale folded into the multiply's key switch (dacapo_amd/csrc/fused_ks.hip f_dr2_icols_lift_fcols_kernel; option ks_fold_rescale,
dc_ct_mul_relin_rescale).  One exact pass divides by P q_{l-1}, so every limb must EQUAL the default path's -- the unchanged oracle is the
reference (tests/test_ks_fold_rescale_oracle.py restates the identity on the CPU):
  * kernel level: dc_ct_mul_relin_rescale == rescale(mul_relin(a, b)) at one kept limb, in the middle and at the top of a 6-prime chain and at
    the reference's ring and top level; with "+ plaintext" and "* constant"; a square; dst aliasing a; every forced launch shape (the folded
    form or the default sequence, whichever the options select); a mixed 60/51-bit chain on the generic-width build;
  * VM level: a program with eligible and ineligible pairs in all four execution modes equals the unchanged oracle VM, the plan reports
    exactly the eligible pairs, and with the option off nothing changes; two streams; max_batch = 2;
  * a prefix of the ResNet-20 program through its first activation: limbs with the option on == limbs with it off."""
import ctypes as C
import gc
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_helpers import _get_ct, _import_keys, _mirror_vm  # noqa: E402
from oracle.oracle import Ciphertext, Oracle, Plaintext, splitmix_fill  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


def _new_symbols():
    """the two entry points this feature adds (an AttributeError where the library or the binding lacks them)"""
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    return ll.lib().dc_ct_mul_relin_rescale, runner.reinit_lw().hevm_last_run_fold_rescale_stats


_RINGS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _release_rings_after_the_module():
    """the rings' contexts and key buffers are shared by this module's tests and freed with it"""
    yield
    _RINGS.clear()
    gc.collect()


def _ring(logN, K, primes=None):
    """oracle with a relinearisation key (host and device) and a context, made once per ring and left unchanged; the last entry caches
    the oracle's results per level"""
    from dacapo_amd import lowlevel as ll

    key = (logN, K, tuple(primes) if primes else None)
    if key not in _RINGS:
        o = Oracle(logN, K, primes=primes)
        o.keygen(seed=0x4845564D, galois_elts=[], relin=True)
        ctx = ll.Context(logN, K) if primes is None else ll.Context(logN, primes=primes)
        assert ctx.primes == o.primes
        _RINGS[key] = (o, ll.DeviceBuffer.from_host(o.relin), ctx, {})
    return _RINGS[key]


def _operand(o, ell, seed):
    q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
    return np.stack([np.stack([splitmix_fill(seed + 7 * p + i + 100 * ell, o.N) for i in range(ell)]) % q for p in range(2)])


def _want(ring, ell, kind="ab"):
    """the oracle's default path on the level's operands, computed once and shared: rescale(mul_relin(a, b)), the same of a square, and
    rescale(mul_plain(add_plain(mul_relin(a, b), A), S)) with S the encoding of the all-ones vector at scale 2^20"""
    o, cache = ring[0], ring[3]
    if (ell, kind) not in cache:
        a, b = Ciphertext(_operand(o, ell, 1), 2.0**40), Ciphertext(_operand(o, ell, 99), 2.0**40)
        if kind == "ab":
            cache[(ell, kind)] = o.rescale(o.mul_relin(a, b)).data
        elif kind == "aa":
            cache[(ell, kind)] = o.rescale(o.mul_relin(a, a)).data
        else:
            A, S = _operand(o, ell, 777)[0], o.encode(np.ones(o.slots), 2.0**20, ell)
            prod = o.mul_relin(a, b)
            cache[(ell, kind)] = (o.rescale(o.mul_plain(o.add_plain(prod, Plaintext(A, prod.scale)), S)).data, A, S.data[:, 0].copy())
    return cache[(ell, kind)]


def _call(ring, ell, square=False, alias=False, add=None, mul=None):
    """dc_ct_mul_relin_rescale on the level's operands -> (result [2][l-1][N], a and b read back afterwards)"""
    from dacapo_amd import lowlevel as ll

    o, dkey, ctx, _ = ring
    N, L = o.N, ctx.L
    a, b = _operand(o, ell, 1), _operand(o, ell, 99)
    da = ll.DeviceBuffer.from_host(a)
    db = da if square else ll.DeviceBuffer.from_host(b)
    dd = da if alias else ll.DeviceBuffer((2, ell - 1, N))
    dst_stride = ell * N if alias else (ell - 1) * N
    dadd = ll.DeviceBuffer.from_host(add) if add is not None else None
    hmul = (C.c_uint64 * ell)(*[int(x) for x in mul]) if mul is not None else None
    L.dc_ct_mul_relin_rescale(ctx.h, dd.ptr, dst_stride, da.ptr, ell * N, db.ptr, ell * N, dkey.ptr, dadd.ptr if dadd else None, hmul, ell, None)
    L.dc_stream_sync(None)
    got = dd.to_host()
    if alias:
        return np.ascontiguousarray(got[:, : ell - 1]), None, db.to_host()
    return got, da.to_host(), db.to_host()


@pytest.mark.parametrize("logN,K,ell", [(12, 6, 2), (12, 6, 3), (12, 6, 5), (15, 14, 13)])
def test_mul_relin_rescale_equals_the_oracle(logN, K, ell):
    """l = 2: one kept limb, the smallest shape the kernels have; l = 5: the top of a 6-prime chain; N = 2^15, l = 13: the reference ring.
    The operands are unchanged afterwards."""
    _new_symbols()
    ring = _ring(logN, K)
    got, a, b = _call(ring, ell)
    assert (got == _want(ring, ell)).all()
    assert (a == _operand(ring[0], ell, 1)).all() and (b == _operand(ring[0], ell, 99)).all()


def test_with_added_plaintext_and_constant_multiplier():
    _new_symbols()
    ring = _ring(12, 6)
    want, A, s = _want(ring, 3, "full")
    got, _, _ = _call(ring, 3, add=A, mul=s)
    assert (got == want).all()
    # each of the two alone: A = 0 / s = 1 are the absent forms
    o = ring[0]
    a, b = Ciphertext(_operand(o, 3, 1), 2.0**40), Ciphertext(_operand(o, 3, 99), 2.0**40)
    prod = o.mul_relin(a, b)
    got, _, _ = _call(ring, 3, add=A)
    assert (got == o.rescale(o.add_plain(prod, Plaintext(A, prod.scale))).data).all()
    got, _, _ = _call(ring, 3, mul=s)
    assert (got == o.rescale(o.mul_plain(prod, o.encode(np.ones(o.slots), 2.0**20, 3))).data).all()


@pytest.mark.parametrize("ell", [2, 3])
def test_square_and_aliased_destination(ell):
    """a and b the same pointer; dst the same pointer as a (the first l - 1 limbs of each polynomial of a are overwritten, b is unchanged)"""
    _new_symbols()
    ring = _ring(12, 6)
    got, _, _ = _call(ring, ell, square=True)
    assert (got == _want(ring, ell, "aa")).all()
    got, _, b = _call(ring, ell, alias=True)
    assert (got == _want(ring, ell)).all()
    assert (b == _operand(ring[0], ell, 99)).all()
    got, _, _ = _call(ring, ell, square=True, alias=True)
    assert (got == _want(ring, ell, "aa")).all()


@pytest.mark.parametrize("opts", [dict(tiny_tile_wgs=0, small_tile_wgs=0), dict(tiny_tile_wgs=0, small_tile_wgs=1 << 30), dict(tiny_tile_wgs=100000),
                                  dict(tiny_tile_wgs=0, small_tile_wgs=0, wide_tile_wgs=0, ks_big_tiles=0), dict(wide_tile_wgs=-1, ks_big_tiles=0),
                                  dict(ks_fuse_mac=0), dict(ks_fuse_mac=1), dict(ks_items_fast=0), dict(ks_items_fast=1),
                                  dict(ks_big_tiles=0, ks_merge_lift_min_wgs=0), dict(tiny_tile_wgs=0, ks_merge_lift_min_wgs=0),
                                  dict(ks_merge_special_min_wgs=0), dict(ks_merge_special_min_wgs=0, tiny_tile_wgs=0),
                                  dict(ks_big_tiles=1), dict(ks_fuse_mac_tiles=0), dict(ks_merge_lift_min_wgs=0, ks_merge_special_min_wgs=0)])
def test_under_every_forced_launch_shape(opts):
    """N = 2^12, l = 3: the thresholds tests/test_gpu_ks_hoist.py forces, plus ks_big_tiles = 1 and the un-fused middle.  The tile geometries,
    the merged inverse phase of the two-limb COLS kernel, both special-prime accumulators in one workgroup row -- or, where the default
    sequence takes its large-batch form or the un-fused middle, that sequence: the limbs are equal either way."""
    _new_symbols()
    from dacapo_amd import runner

    ring = _ring(12, 6)
    want, A, s = _want(ring, 3, "full")
    with runner.options(**opts):
        got, _, _ = _call(ring, 3)
        full, _, _ = _call(ring, 3, add=A, mul=s)
    assert (got == _want(ring, 3)).all(), opts
    assert (full == want).all(), opts


def test_mixed_width_chain_on_the_generic_width_build():
    """60-bit base and special primes around 51-bit rescale primes, (12, 6, 3): the lifts between width classes"""
    _new_symbols()
    from test_gpu_prime_widths import _chain

    from dacapo_amd import lowlevel as ll

    primes = _chain(12, [60, 51, 51, 51, 51, 60])
    ring = _ring(12, 6, primes=primes)
    assert ring[2].L is ll.lib_gw()
    got, _, _ = _call(ring, 3)
    assert (got == _want(ring, 3)).all()
    want, A, s = _want(ring, 3, "full")
    full, _, _ = _call(ring, 3, add=A, mul=s)
    assert (full == want).all()


# ---- VM level ---------------------------------------------------------------------------------------------------------------------------
PAIRS = 7  # the pairs _program is built to contain that qualify: 3 ciphertexts x 2 rounds, and the pair whose rescale is a program output


def _program(slots, seed=23):
    """three independent ciphertexts through two rounds of mulcc -> addcp -> mulcp(all-ones) -> rescale (the second round multiplies the first's
    result: by itself, by another input, by itself); one mulcc -> mulcp(all-ones) -> rescale whose product has a second reader; one mulcc ->
    mulcp(a non-constant vector) -> rescale; one merged-shape pair whose rescale result is a program output.  The ineligible pairs sit at levels
    of their own: a step is merged only when every item of it qualifies."""
    from dacapo_amd import hevm_asm as ha

    rng = np.random.default_rng(seed)
    b = ha.Builder(slots=slots, init_level=5, policy="eager", shadow=True)
    x = [b.input(rng.uniform(-1, 1, slots)) for _ in range(3)]
    w = [b.input(rng.uniform(-1, 1, slots), level=4) for _ in range(2)]
    u = [b.input(rng.uniform(-1, 1, slots), level=3) for _ in range(2)]
    v = [b.input(rng.uniform(-1, 1, slots), level=2) for _ in range(2)]

    def merged_shape(p, q):
        return b.rescale(b.upscale(b.add_plain(b.mul(p, q), rng.uniform(-1, 1, slots)), 20))

    r1 = [merged_shape(x[0], x[0]), merged_shape(x[1], x[2]), merged_shape(x[2], x[0])]
    r2 = [merged_shape(r1[0], r1[0]), merged_shape(r1[1], w[0]), merged_shape(r1[2], r1[2])]
    for r in r2:
        b.output(r)
    m = b.mul(u[0], u[1])                       # a second reader: the product itself is negated and returned
    b.output(b.rescale(b.upscale(m, 20)))
    b.output(b.negate(m))
    nc = b.mul_plain(b.mul(v[0], v[1]), rng.uniform(0.5, 1, slots), scale_bits=20, normalise=False)  # not a constant polynomial
    b.output(b.rescale(nc))
    b.output(merged_shape(w[0], w[1]))          # eligible: the RESCALE's result may be an output, the product may not
    return b


def _run_program(tmp_path, fold, plan=1, graph=1, streams=1, extra=None):
    """the program on a VM with ks_fold_rescale = fold; every result register of every stream against the unchanged oracle VM on the same
    key / plaintext / input limbs -> the pair count of the run"""
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    logN, K = 12, 6
    opts = {"plan": plan, "plan_graph": graph, "ks_fold_rescale": fold}
    opts.update(extra or {})
    hevm = runner.HEVM(seed=77, logN=logN, num_primes=K, vm_options=opts)
    o = Oracle(logN, K)
    _import_keys(o, hevm, ll)
    if streams > 1:
        hevm.set_streams(streams)
    b = _program(1 << (logN - 1))
    cst, hv, _ = b.assemble()
    hevm.load_mem(cst, hv)
    ovms = []
    for s in range(streams):
        hevm.select_stream(s)
        ovm = _mirror_vm(hevm, ll, o, cst, hv, tmp_path)
        for i, a in enumerate(b.args):
            hevm.setInput(i, a.plain * (1.0 - 0.25 * s))
            ovm.ciphers[i] = _get_ct(hevm, ll, i)
        ovms.append(ovm)
    hevm.run()
    for s, ovm in enumerate(ovms):
        hevm.select_stream(s)
        ovm.run()
        assert len(ovm.prog.res_dst) == 7
        for r in ovm.prog.res_dst:
            got, want = _get_ct(hevm, ll, r), ovm.ciphers[r]
            assert got.ell == want.ell and got.scale == want.scale, (s, r)
            assert (got.data == want.data).all(), (s, r)
    hevm.select_stream(0)
    if streams == 1:
        for got, want in zip(hevm.getOutput(), b.expected()):
            assert np.abs(got - want).max() < 1e-4
    st = hevm.stats()
    assert st["op_counts"][8] == 9 and st["op_counts"][3] == 9  # a merged step still counts as one multiply and one rescale
    pairs = hevm.fold_rescale_stats()
    hevm.close()
    return pairs, st


@pytest.mark.parametrize("plan,graph", [(1, 1), (1, 0), (0, 1), (1, 2)])
def test_vm_program_equals_the_unchanged_oracle_vm(tmp_path, plan, graph):
    """plan + graph, plan without graph, the loop, the explicitly built graph: every result register == OracleVM; the plan modes merge exactly
    the pairs the program was built to contain (the pair with a second reader and the one with a non-constant multiplier are not counted);
    the loop stays on the two calls"""
    _new_symbols()
    pairs, st = _run_program(tmp_path, 1, plan, graph)
    assert pairs == (PAIRS if plan else 0)
    off, st0 = _run_program(tmp_path, 0, plan, graph)
    assert off == 0
    assert st["keyswitches"] == st0["keyswitches"] and st["ntts"] == st0["ntts"]  # the NTT-equivalent count stays the default's


def test_two_streams_with_different_inputs(tmp_path):
    """each stream equals its own oracle run; an item is a pair of one stream"""
    _new_symbols()
    assert _run_program(tmp_path, 1, streams=2)[0] == 2 * PAIRS


def test_max_batch_two(tmp_path):
    """the three-item steps are cut into two: multiply and rescale steps are cut alike, so the pairs stay pairs"""
    _new_symbols()
    assert _run_program(tmp_path, 1, extra={"max_batch": 2})[0] == PAIRS


def test_resnet20_prefix_limbs_equal_with_the_option_on_and_off():
    """the ResNet-20 program through its first activation (cut before the rotations of the next convolution; 19 ct x ct multiplies, 16 opcode
    10 whose zero-encryptions the test hook makes (0, 0)): the result limbs with ks_fold_rescale = 1 == those with 0, at least 6 pairs merged"""
    _new_symbols()
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
    ops = ha.unpack_hevm(fx["hevm"])["ops"]
    first_boot = int(np.nonzero(ops[:, 0] == ha.OP_BOOTSTRAP)[0][0])
    cut = first_boot + int(np.nonzero(ops[first_boot:, 0] == ha.OP_ROTATE)[0][0])
    assert (ops[:cut, 0] == ha.OP_MULCC).sum() >= 10
    hv, lvl, _ = ha.truncate_hevm(fx["hevm"], cut)
    res = {}
    for fold in (0, 1):
        hevm = runner.HEVM(seed=0x4845564D, logN=15, num_primes=14, vm_options={"ks_fold_rescale": fold})
        hevm.lw.hevm_test_zero_encryption(hevm.vm, True)
        hevm.load_mem(fx["cst"], hv)
        hevm.setInput(0, fx["packed"])
        hevm.run()
        reg = int(ha.unpack_hevm(hv)["res_dst"][0])
        res[fold] = (_get_ct(hevm, ll, reg), hevm.fold_rescale_stats())
        hevm.close()
    (off, n_off), (on, n_on) = res[0], res[1]
    print(f"ResNet-20 prefix of {cut} instructions: {n_on} pairs merged")
    assert n_off == 0 and n_on >= 6
    assert on.ell == off.ell == lvl and on.scale == off.scale
    assert (on.data == off.data).all()
