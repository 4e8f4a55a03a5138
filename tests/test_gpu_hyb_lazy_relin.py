"""GPU: lazy relinearisation under grouped-digit keys (dacapo_amd/csrc/hybrid_fused.hip hybf_irows_tensor_sum_kernel /
hybf_frows_sum_final_kernel, hybrid_ks.hip hyb_mul_sum_relin; dc_ct_mul_sum_relin on a grouped-digit context, option hyb_lazy_relin).
The definition, on the unchanged oracle under set_hybrid(ks, alpha): T = sum_k s_k Oracle.tensor(a_k, b_k) by poly_add / poly_sub, then
Oracle.keyswitch(T2, relin, T0, T1); every limb compared with ==.  Rings, operands, terms, the program and its replay are the neighbours'."""
import subprocess
import sys

import numpy as np
import pytest

from gpu_helpers import _get_ct, _import_keys, _mirror_vm
from oracle.oracle import Oracle
from test_gpu_hyb_fold_rescale import LOGN, _ring
from test_gpu_lazy_relin import CAP, _call_sum, _define, _operand, _replay_vm, _terms, _vm_program

pytestmark = pytest.mark.gpu
_KNOWN: list = []


def _option_known():
    """hevm_get_option aborts on a name the library lacks, so the question is put by a child process, once"""
    if not _KNOWN:
        r = subprocess.run([sys.executable, "-c", "from dacapo_amd import runner; print(runner.get_option('hyb_lazy_relin'))"], capture_output=True, text=True)
        _KNOWN.append((r.returncode, r.stdout.strip()))
    return _KNOWN[0]


def _check(ring, ell, terms, dst=None):
    """dc_ct_mul_sum_relin == the definition; every operand that is not the destination is unchanged"""
    assert _option_known() == (0, "0"), "hyb_lazy_relin is no option of this library: it refuses a grouped-digit context here"
    got, ops = _call_sum(ring, ell, terms, dst=dst)
    assert (got == _define(ring, ell, terms)).all(), (ell, terms, dst)
    for w, v in ops.items():
        assert (v == _operand(ring[0], ell, w)).all(), (ell, terms, dst, w)


# levels 1, 2, 3, 5: one partial digit, one full, full + partial, two full + partial (matrix-core conversion under hyb_fuse = 2); counts: 9
# crosses the fold interval, 32 is the cap.  Every count and level at (8, 3, 2), fused; other sequences / key shapes at 3 products, long walks at l = 5
SHAPES = ([(8, 3, 2, ell, 1, n) for ell in (1, 2, 3, 5) for n in (1, 2, 3, 9, CAP)]
          + [(8, 3, 2, ell, fuse, 3) for ell in (1, 2, 3, 5) for fuse in (2, 0)] + [(8, 3, 2, 5, fuse, n) for fuse in (2, 0) for n in (9, CAP)]
          + [(K, ks, alpha, ell, fuse, 3) for K, ks, alpha in ((7, 2, 2), (14, 9, 8)) for ell in (1, 2, 3, 5) for fuse in (1, 2, 0)])


@pytest.mark.parametrize("K,ks,alpha,ell,fuse,count", SHAPES)
def test_mul_sum_relin_equals_the_definition(K, ks, alpha, ell, fuse, count):
    from dacapo_amd import runner

    with runner.options(hyb_fuse=fuse):
        _check(_ring(K, ks, alpha), ell, _terms(count))


@pytest.mark.parametrize("ell", [1, 3])
def test_one_product_is_mul_relin(ell):
    from dacapo_amd import lowlevel as ll

    assert _option_known()[0] == 0
    o, dkey, ctx, _ = ring = _ring(8, 3, 2)
    st = ell * o.N
    got, _ = _call_sum(ring, ell, [(0, 1, 1)])
    da, db, dm = ll.DeviceBuffer.from_host(_operand(o, ell, 0)), ll.DeviceBuffer.from_host(_operand(o, ell, 1)), ll.DeviceBuffer((2, ell, o.N))
    ctx.L.dc_ct_mul_relin(ctx.h, dm.ptr, st, da.ptr, st, db.ptr, st, dkey.ptr, ell, None)
    ctx.L.dc_stream_sync(None)
    assert (got == dm.to_host()).all()


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("terms,dst", [([(0, 0, 1), (1, 1, -1)], None),             # squares
                                       ([(0, 1, 1), (0, 2, 1), (2, 0, -1)], None),   # one operand in every term, on either side
                                       ([(0, 1, 1), (2, 3, -1)], 0),                 # dst is an a operand
                                       ([(0, 1, 1), (2, 3, -1), (3, 3, 1)], 3),      # dst is a b operand and both sides of a square
                                       ([(0, 0, 1)], 0)])                            # one square onto itself
def test_squares_shared_operands_and_an_aliased_destination(terms, dst, fuse):
    from dacapo_amd import runner

    with runner.options(hyb_fuse=fuse):
        _check(_ring(8, 3, 2), 3, terms, dst)


@pytest.mark.parametrize("signs", ["plus", "alternating", "two_to_one"])
@pytest.mark.parametrize("ell", [1, 5])
def test_extreme_operands_at_the_largest_count(ell, signs):
    """every limb q_i - 1, CAP terms: 16 products of (q - 1)^2 between two folds on the c1 component, in one accumulator or split over both"""
    period = {"plus": 1, "alternating": 2, "two_to_one": 3}[signs]
    _check(_ring(8, 3, 2), ell, [("max", "max", -1 if (period > 1 and k % period == period - 1) else 1) for k in range(CAP)])


def test_mixed_width_chain_on_the_generic_width_build():
    from test_gpu_prime_widths import _chain

    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    ring = _ring(6, 2, 2, primes=_chain(LOGN, [60, 51, 51, 51, 60, 60]))
    assert ring[2].L is ll.lib_gw()
    for fuse in (1, 0):
        with runner.options(hyb_fuse=fuse):
            _check(ring, 3, _terms(9))


def _run_vm(tmp_path, lazy, plan=1, graph=1, streams=1):
    """tests/test_gpu_lazy_relin.py's program on a grouped-digit VM: every result of every stream == the replay of the exported groups (none:
    the plain OracleVM) -> (groups, the groups the program holds, relin stats, max slot error per output of stream 0, result limbs)"""
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    assert _option_known() == (0, "0"), "hyb_lazy_relin is no option of this library"
    K, ks = 7, 2
    hevm = runner.HEVM(seed=91, logN=LOGN, num_primes=K, ks_special=ks, ks_alpha=ks, vm_options={"plan": plan, "plan_graph": graph, "hyb_lazy_relin": lazy})
    o = Oracle(LOGN, K)
    o.set_hybrid(ks, ks)
    _import_keys(o, hevm, ll, elts=[])
    if streams > 1:
        hevm.set_streams(streams)
    b, want_groups = _vm_program(1 << (LOGN - 1))
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
    hevm.run()
    groups, limbs = hevm.relin_groups(), []
    for s, ovm in enumerate(ovms):
        hevm.select_stream(s)
        if isinstance(groups, list):
            ovm.set_relin_groups(groups)
        ovm.run()
        assert len(ovm.prog.res_dst) == 7
        for r in ovm.prog.res_dst:
            got, want = _get_ct(hevm, ll, r), ovm.ciphers[r]
            assert got.ell == want.ell and got.scale == want.scale and (got.data == want.data).all(), (s, r)
            limbs.append(got.data)
    hevm.select_stream(0)
    errs = [float(np.abs(got - want).max()) for got, want in zip(hevm.getOutput(), b.expected())]
    rst = hevm.relin_stats()
    hevm.close()
    return groups, want_groups, rst, errs, limbs


@pytest.mark.parametrize("graph,streams", [(1, 1), (0, 1), (1, 2)])
def test_vm_groups_limbs_and_error(tmp_path, graph, streams):
    """option on: the program's two groups, limbs == their oracle replay, slot error within 2 x the option-off run's (the SEAL-layout bound)"""
    groups, want, rst, errs, _ = _run_vm(tmp_path, 1, 1, graph, streams)
    assert groups == want and rst == {"groups": 2 * streams, "products": 6 * streams}
    g0, _, rst0, errs0, _ = _run_vm(tmp_path, 0, 1, graph, streams)
    assert g0 == 0 and rst0 == {"groups": 0, "products": 0}
    for k, (e1, e0) in enumerate(zip(errs, errs0)):
        assert e1 <= 2 * e0, f"output {k}: lazy {e1:.3e} against default {e0:.3e} (bound 2 x)"


def test_vm_loop_ignores_the_option(tmp_path):
    groups, _, rst, _, on = _run_vm(tmp_path, 1, plan=0)
    assert groups == -1 and rst == {"groups": 0, "products": 0}
    _, _, _, _, off = _run_vm(tmp_path, 0, plan=0)
    assert all((x == y).all() for x, y in zip(on, off))
