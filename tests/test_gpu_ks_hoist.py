"""GPU: hoisted rotations on SEAL-layout keys (dacapo_amd/csrc/hoist_ks.hip; option ks_hoist, dc_ct_rotate_hoisted) against the oracle's
orc_rotate_ks_hybrid at one special prime and one prime per digit, limb for limb (tests/test_ks_hoist_oracle.py shows that this function is a
correct rotation and is not SEAL's hop):
  * kernel level: a single hop at levels without a cross-prime lift, in the middle and at the top of the chain, and at the reference's ring
    and top level; five hops of one source on one decomposition equal five single hops bit for bit; every forced launch shape;
  * VM level: a convolution-shaped program in all four execution modes equals an oracle VM whose hop is the hoisted definition, the run
    statistics report the shared decompositions, and with the option off nothing changes;
  * the option is refused where it is meaningless (grouped digits), and the ResNet-20 inference still decrypts to the torch logits."""
import ctypes as C
import gc
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_helpers import _get_ct, _import_keys, _mirror_vm  # noqa: E402
from oracle.oracle import Ciphertext, Oracle, OracleVM, _p, splitmix_fill  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
STEPS = [1, -3, 0, 5, 2]  # 0: the conjugation (element 2N - 1)


def _new_symbols():
    """the two entry points this feature adds (an AttributeError where the library or the binding lacks them)"""
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    return ll.lib().dc_ct_rotate_hoisted, runner.reinit_lw().hevm_last_run_hoist_stats


class HoistOracle(Oracle):
    """an oracle whose key-switch hop is the hoisted definition: digits of c1 before the automorphism (orc_rotate_ks_hybrid on a context
    left at one special prime, one prime per digit)"""

    def apply_galois(self, a: Ciphertext, elt: int) -> Ciphertext:
        assert (self.ks, self.alpha) == (1, 1)
        c0 = self.galois_ntt(a.data[0], elt)
        c1 = np.zeros_like(c0)
        key = self.galois[elt]
        assert key.shape == (self.K - 1, 2, self.K, self.N)
        self.L.orc_rotate_ks_hybrid(self.ctx, a.ell, _p(np.ascontiguousarray(a.data[1])), C.c_uint32(elt), _p(key), _p(c0), _p(c1))
        return Ciphertext(np.stack([c0, c1]), a.scale)


_RINGS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _release_rings_after_the_module():
    """the rings' contexts, key buffers and hoisting scratch (about 1 GB of HBM at N = 2^15) are shared by this module's tests and freed with
    it: the modules that follow find the device as they would without this one"""
    yield
    _RINGS.clear()
    gc.collect()


def _ring(logN, K):
    """oracle, keys of the five elements (host and device) and a context, made once per ring and left unchanged"""
    from dacapo_amd import lowlevel as ll

    if (logN, K) not in _RINGS:
        o = HoistOracle(logN, K)
        elts = [o.elt_from_step(s) for s in STEPS]
        o.keygen(seed=0x4845564D, galois_elts=elts, relin=False)
        ctx = ll.Context(logN, K)
        assert ctx.primes == o.primes
        _RINGS[(logN, K)] = (o, elts, {e: ll.DeviceBuffer.from_host(o.galois[e]) for e in elts}, ctx, {})
    return _RINGS[(logN, K)]


def _source(o, ell):
    q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
    return np.stack([np.stack([splitmix_fill(1 + 7 * p + i + 100 * ell, o.N) for i in range(ell)]) % q for p in range(2)])


def _want(ring, ell, elt):
    """the oracle's hop of the level's source, computed once and shared"""
    o, cache = ring[0], ring[4]
    if (ell, elt) not in cache:
        cache[(ell, elt)] = o.apply_galois(Ciphertext(_source(o, ell), 2.0**40), elt).data
    return cache[(ell, elt)]


def _hoisted(ring, ell, elts, src=None):
    """dc_ct_rotate_hoisted of the level's source for `elts` in one call -> (outputs, source read back afterwards)"""
    from dacapo_amd import lowlevel as ll

    o, _, dkeys, ctx, _ = ring
    n, N = len(elts), o.N
    a = _source(o, ell) if src is None else src
    da = ll.DeviceBuffer.from_host(a)
    outs = [ll.DeviceBuffer((2, ell, N)) for _ in elts]
    dsts = (C.c_void_p * n)(*[d.ptr for d in outs])
    keys = (C.c_void_p * n)(*[dkeys[e].ptr for e in elts])
    ge = (C.c_uint32 * n)(*elts)
    ll.lib().dc_ct_rotate_hoisted(ctx.h, dsts, ell * N, da.ptr, ell * N, ge, keys, n, ell, None)
    ll.lib().dc_stream_sync(None)
    return [d.to_host() for d in outs], da.to_host()


@pytest.mark.parametrize("logN,K,ell,opts", [(12, 6, 1, {}), (12, 6, 2, {}), (12, 6, 3, {}), (12, 6, 5, {}), (15, 14, 13, {}),
                                             (15, 14, 13, {"small_tile_wgs": 0, "wide_tile_wgs": 0})])
def test_single_hoisted_hop_equals_the_oracle(logN, K, ell, opts):
    """count = 1.  l = 1: no cross-prime lift (one digit, raised to the special prime only); l = 5: the top of a 6-prime chain; N = 2^15,
    l = 13: the large-batch lift, and (second set) its radix-16 tiles, which batches of several sources take by themselves.  Step 1, step -3,
    conjugation."""
    _new_symbols()
    from dacapo_amd import runner

    ring = _ring(logN, K)
    with runner.options(**opts):
        for elt in ring[1][:3]:
            (got,), _ = _hoisted(ring, ell, [elt])
            assert (got == _want(ring, ell, elt)).all(), (ell, elt)


@pytest.mark.parametrize("logN,K,ell", [(12, 6, 3), (15, 14, 13)])
def test_five_hops_share_one_decomposition(logN, K, ell):
    """five elements of one source in one call: every output equals the oracle and the count = 1 call (sharing changes no limb), and the
    source is unchanged"""
    _new_symbols()
    ring = _ring(logN, K)
    elts = ring[1]
    src = _source(ring[0], ell)
    outs, after = _hoisted(ring, ell, elts)
    assert (after == src).all()
    for elt, got in zip(elts, outs):
        assert (got == _want(ring, ell, elt)).all(), elt
        (single,), _ = _hoisted(ring, ell, [elt])
        assert (got == single).all(), elt


@pytest.mark.parametrize("opts", [dict(tiny_tile_wgs=0, small_tile_wgs=0), dict(tiny_tile_wgs=0, small_tile_wgs=1 << 30), dict(tiny_tile_wgs=100000),
                                  dict(tiny_tile_wgs=0, small_tile_wgs=0, wide_tile_wgs=0, ks_big_tiles=0), dict(wide_tile_wgs=-1, ks_big_tiles=0),
                                  dict(ks_fuse_mac=0), dict(ks_fuse_mac=1), dict(ks_items_fast=0), dict(ks_items_fast=1),
                                  dict(ks_big_tiles=0, ks_merge_lift_min_wgs=0), dict(tiny_tile_wgs=0, ks_merge_lift_min_wgs=0),
                                  dict(ks_merge_special_min_wgs=0), dict(ks_merge_special_min_wgs=0, tiny_tile_wgs=0)])
def test_hoisted_hops_under_every_forced_launch_shape(opts):
    """N = 2^12, l = 3, one hop and five: the tile geometries (radix-8 / radix-4 / one-butterfly by option; everything at this size is below
    tiny_tile_wgs by default), the large-batch lift and the latency form with the merged inverse phase, both special-prime accumulators in one workgroup row, items faster or slower than rows"""
    _new_symbols()
    from dacapo_amd import runner

    ring = _ring(12, 6)
    elts = ring[1]
    with runner.options(**opts):
        for elt in elts[:3]:
            (got,), _ = _hoisted(ring, 3, [elt])
            assert (got == _want(ring, 3, elt)).all(), (opts, elt)
        outs, _ = _hoisted(ring, 3, elts)
    for elt, got in zip(elts, outs):
        assert (got == _want(ring, 3, elt)).all(), (opts, elt)


def _conv_program(slots, levels):
    """two layers of: one input rotated by 1, 2, 3, 5 (two-hop NAF offsets under the default keys) and -1, each times a plaintext, summed with a
    second input rotated by 1 and 4; a rescale between them.  Returns the builder and the rotations as (source value id, offset)."""
    from dacapo_amd import hevm_asm as ha

    rng = np.random.default_rng(17)
    b = ha.Builder(slots=slots, init_level=levels, policy="lazy", boot_level=levels, shadow=True)
    x, y = b.input(rng.uniform(-1, 1, slots)), b.input(rng.uniform(-1, 1, slots))
    rots = []

    def layer(u, v):
        acc = None
        for src, offs in ((u, (1, 2, 3, 5, -1)), (v, (1, 4))):
            for k in offs:
                rots.append((src.id, k))
                t = b.mul_plain(b.rotate(src, k), rng.uniform(-0.5, 0.5, slots))
                acc = t if acc is None else b.add(acc, t)
        return b.rescale(acc)

    r = layer(x, y)
    r2 = b.rescale(b.mul_plain(y, rng.uniform(-0.5, 0.5, slots)))
    b.output(b.finish(layer(r, r2)))
    return b, rots


@pytest.mark.parametrize("hoist", [1, 0])
@pytest.mark.parametrize("plan,graph", [(1, 1), (1, 0), (0, 1), (1, 2)])
def test_vm_program_equals_the_hoisted_oracle_vm(tmp_path, plan, graph, hoist):
    """ks_hoist = 1: every result limb equals the oracle VM whose hop is the hoisted definition, and the plan computes one decomposition per
    distinct hop source (the loop, plan = 0, executes one hop at a time: one each).  ks_hoist = 0: the unmodified oracle VM, one each."""
    _new_symbols()
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    logN, K = 12, 6
    hevm = runner.HEVM(seed=77, logN=logN, num_primes=K, vm_options={"plan": plan, "plan_graph": graph, "ks_hoist": hoist})
    o = (HoistOracle if hoist else Oracle)(logN, K)
    _import_keys(o, hevm, ll)
    b, rots = _conv_program(1 << (logN - 1), K - 1)
    cst, hv, _ = b.assemble()
    hevm.load_mem(cst, hv)
    ovm = _mirror_vm(hevm, ll, o, cst, hv, tmp_path)
    for i, a in enumerate(b.args):
        hevm.setInput(i, a.plain)
        ovm.ciphers[i] = _get_ct(hevm, ll, i)
    hevm.run()
    ovm.run()
    r = ovm.prog.res_dst[0]
    got, want = _get_ct(hevm, ll, r), ovm.ciphers[r]
    assert got.ell == want.ell and got.scale == want.scale
    assert (got.data == want.data).all()
    assert np.abs(hevm.getOutput()[0] - b.expected()[0]).max() < 1e-5
    # Every hop of a rotation reads either the rotated value or the previous hop's result, which nothing else reads; all the hops that read
    # one value sit in one wave (they depend on that value alone) at one level: one plan step, one decomposition per distinct source.
    hops = sum(len(o.rotate_hops(k)) for _, k in rots)
    sources = len({v for v, _ in rots}) + sum(len(o.rotate_hops(k)) - 1 for _, k in rots)
    assert hops == 18 and sources == 8
    st = hevm.hoist_stats()
    print(plan, graph, hoist, st)
    assert st["hops"] == hops
    if hoist and plan:
        assert st["decompositions"] == sources and st["decompositions"] < st["hops"]
    else:
        assert st["decompositions"] == st["hops"]
    hevm.close()


def test_ks_hoist_is_refused_with_grouped_digits():
    """ks_hoist = 1 with ks_special = 2 aborts at VM creation, before anything is allocated or launched (a child process: the library aborts)"""
    _new_symbols()
    code = ("from dacapo_amd import runner\n"
            "runner.HEVM(fresh=True, logN=12, num_primes=6, ks_special=2, vm_options={'ks_hoist': 1})\n"
            "print('created')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "created" not in r.stdout, (r.returncode, r.stdout)
    assert "ks_hoist" in r.stderr and "ks_special = 2" in r.stderr, r.stderr


def test_resnet20_with_hoisted_rotations_matches_torch():
    """the headline fixture with ks_hoist = 1 decrypts to the torch logits within the bound tests/test_gpu_resnet20.py applies to the default
    run (rms < 3e-3), and its plan shares decompositions"""
    _new_symbols()
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
    hevm = runner.HEVM(seed=0x4845564D, logN=15, num_primes=14, vm_options={"ks_hoist": 1})
    hevm.load_mem(fx["cst"], fx["hevm"])
    hevm.setInput(0, fx["packed"])
    hevm.run()
    out = hevm.getOutput()[0]
    logits, want = out[:10] * 32, fx["torch_result"]
    rms_torch = float(np.sqrt(np.mean((logits - want) ** 2)))
    st = hevm.hoist_stats()
    print(f"ResNet-20 with ks_hoist = 1: rms vs torch {rms_torch:.3e}; {st['hops']} hops on {st['decompositions']} decompositions")
    assert int(np.argmax(logits)) == int(np.argmax(want))
    assert rms_torch < 3e-3
    assert 0 < st["decompositions"] < st["hops"]
    hevm.close()
