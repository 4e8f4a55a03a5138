"""GPU: a rescale folded into the grouped-digit multiply's mod-down (dacapo_amd/csrc/hybrid_fused.hip hybf_mul_relin_rescale_tail; option
hyb_fold_rescale, dc_ct_mul_relin_rescale on a grouped-digit context).  Nothing is rounded differently: every limb == the unchanged oracle's
rescale(mul_relin(a, b)) under the same (ks_special, ks_alpha); tests/test_hyb_fold_rescale_oracle.py restates the identity on the CPU."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from gpu_helpers import _get_ct, _import_keys, _mirror_vm
from oracle.oracle import Ciphertext, Oracle, Plaintext, splitmix_fill

pytestmark = pytest.mark.gpu
LOGN = 12
_RINGS: dict = {}
_KNOWN: list = []


def _option_known():
    """hevm_get_option aborts on a name the library lacks, so the question is put by a child process, once"""
    if not _KNOWN:
        r = subprocess.run([sys.executable, "-c", "from dacapo_amd import runner; print(runner.get_option('hyb_fold_rescale'))"], capture_output=True, text=True)
        _KNOWN.append((r.returncode, r.stdout.strip()))
    return _KNOWN[0]


def test_the_option_exists_and_ships_off():
    assert _option_known() == (0, "0")


def _ring(K, ks, alpha, primes=None):
    """oracle, device relinearisation key, context and the oracle's results per (level, form): made once, left unchanged"""
    from dacapo_amd import lowlevel as ll

    if (K, ks, alpha) not in _RINGS:
        o = Oracle(LOGN, K, primes=primes)
        o.set_hybrid(ks, alpha)
        o.keygen(seed=0x4845564D, galois_elts=[], relin=True)
        ctx = ll.Context(LOGN, K, primes=primes, special=ks, alpha=alpha)
        assert ctx.primes == o.primes and ctx.key_digits == o.dnum
        _RINGS[K, ks, alpha] = (o, ll.DeviceBuffer.from_host(o.relin), ctx, {})
    return _RINGS[K, ks, alpha]


def _operands(o, ell, form):
    q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
    a, b = (np.stack([np.stack([splitmix_fill(s + 7 * p + i + 100 * ell, o.N) for i in range(ell)]) % q for p in range(2)]) for s in (1, 99))
    if form == "edge":  # every limb of both operands at q - 1
        a[:], b[:] = q - np.uint64(1), q - np.uint64(1)
    return a, (a if form == "aa" else b)


def _want(ring, ell, form):
    """the oracle's default pair: rescale(mul_plain(add_plain(mul_relin(a, b), A), S)), A / S only where `form` names them"""
    o, cache = ring[0], ring[3]
    if (ell, form) not in cache:
        a, b = _operands(o, ell, form)
        m = o.mul_relin(Ciphertext(a, 2.0**40), Ciphertext(b, 2.0**40))
        A = _operands(o, ell, "ab")[1][1] if "A" in form else None
        S = o.encode(np.ones(o.slots), 2.0**20, ell) if "s" in form else None
        if A is not None:
            m = o.add_plain(m, Plaintext(A, m.scale))
        if S is not None:
            m = o.mul_plain(m, S)
        cache[ell, form] = (o.rescale(m).data, A, None if S is None else S.data[:, 0].copy())
    return cache[ell, form]


def _check(ring, ell, form="ab", alias=False):
    """dc_ct_mul_relin_rescale on the level's operands == the oracle; the operands it may not write are unchanged"""
    from dacapo_amd import lowlevel as ll

    assert _option_known()[0] == 0, "this library refuses a grouped-digit context here"
    o, dkey, ctx, _ = ring
    N, (a, b), (want, A, s) = o.N, _operands(o, ell, form), _want(ring, ell, form)
    da = ll.DeviceBuffer.from_host(a)
    db = da if form == "aa" else ll.DeviceBuffer.from_host(b)
    dd = da if alias else ll.DeviceBuffer((2, ell - 1, N))
    dadd = ll.DeviceBuffer.from_host(A) if A is not None else None
    hmul = (C.c_uint64 * ell)(*[int(x) for x in s]) if s is not None else None
    ctx.L.dc_ct_mul_relin_rescale(ctx.h, dd.ptr, (ell if alias else ell - 1) * N, da.ptr, ell * N, db.ptr, ell * N, dkey.ptr,
                                  dadd.ptr if dadd else None, hmul, ell, None)
    ctx.L.dc_stream_sync(None)
    assert (dd.to_host()[:, : ell - 1] == want).all(), (form, alias)
    assert alias or (da.to_host() == a).all(), form
    assert (alias and form == "aa") or (db.to_host() == b).all(), form


@pytest.mark.parametrize("fuse", [1, 2, 0])
@pytest.mark.parametrize("ell", [2, 3, 5])  # one kept limb; the dropped prime a partial digit of its own; the matrix-core conversion (hyb_fuse = 2)
@pytest.mark.parametrize("K,ks,alpha", [(7, 2, 2), (8, 3, 2), (14, 9, 8)])  # (14, 9, 8): nine special primes, config 4's mod-down
def test_mul_relin_rescale_equals_the_oracle(K, ks, alpha, ell, fuse):
    from dacapo_amd import runner

    with runner.options(hyb_fuse=fuse):
        _check(_ring(K, ks, alpha), ell)


@pytest.mark.parametrize("ell", [3, 5])
@pytest.mark.parametrize("form,alias", [("+A", False), ("*s", False), ("+A*s", False), ("aa", False), ("ab", True), ("aa", True), ("edge", False)])
def test_forms_at_ks3_alpha2(form, alias, ell):
    _check(_ring(8, 3, 2), ell, form, alias)


def test_mixed_width_chain_on_the_generic_width_build():
    from test_gpu_prime_widths import _chain

    from dacapo_amd import lowlevel as ll

    ring = _ring(6, 2, 2, primes=_chain(LOGN, [60, 51, 51, 51, 60, 60]))
    assert ring[2].L is ll.lib_gw()
    _check(ring, 3)
    _check(ring, 3, "+A*s")


def _run_program(tmp_path, fold, plan=1, graph=1, streams=1):
    """tests/test_gpu_ks_fold_rescale.py's program on a grouped-digit VM: every result register of every stream == the oracle VM on the same
    keys -> (merged pairs, stats, the result limbs)"""
    from test_gpu_ks_fold_rescale import _program

    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    assert _option_known()[0] == 0, "hyb_fold_rescale is no option of this library"
    K, ks = 7, 2
    hevm = runner.HEVM(seed=77, logN=LOGN, num_primes=K, ks_special=ks, ks_alpha=ks, vm_options={"plan": plan, "plan_graph": graph, "hyb_fold_rescale": fold})
    o = Oracle(LOGN, K)
    o.set_hybrid(ks, ks)
    _import_keys(o, hevm, ll, elts=[])
    if streams > 1:
        hevm.set_streams(streams)
    b = _program(1 << (LOGN - 1))
    cst, hv, _ = b.assemble()
    hevm.load_mem(cst, hv)
    ovms = []
    for s in range(streams):
        hevm.select_stream(s)
        ovms.append(_mirror_vm(hevm, ll, o, cst, hv, tmp_path))
        for i, a in enumerate(b.args):
            hevm.setInput(i, a.plain * (1.0 - 0.25 * s))
            ovms[s].ciphers[i] = _get_ct(hevm, ll, i)
    hevm.run()
    limbs = []
    for s, ovm in enumerate(ovms):
        hevm.select_stream(s)
        ovm.run()
        assert len(ovm.prog.res_dst) == 7
        for r in ovm.prog.res_dst:
            got, want = _get_ct(hevm, ll, r), ovm.ciphers[r]
            assert got.ell == want.ell and got.scale == want.scale and (got.data == want.data).all(), (s, r)
            limbs.append(got.data)
    st, pairs = hevm.stats(), hevm.fold_rescale_stats()
    assert st["op_counts"][8] == 9 and st["op_counts"][3] == 9  # a merged step still counts as one multiply and one rescale
    hevm.close()
    return pairs, st, limbs


@pytest.mark.parametrize("plan,graph,streams", [(1, 1, 1), (1, 0, 1), (0, 1, 1), (1, 1, 2)])
def test_vm_program_equals_the_oracle_vm_and_merges_the_built_in_pairs(tmp_path, plan, graph, streams):
    from test_gpu_ks_fold_rescale import PAIRS

    pairs, st, on = _run_program(tmp_path, 1, plan, graph, streams)
    assert pairs == (streams * PAIRS if plan else 0)
    none, st0, off = _run_program(tmp_path, 0, plan, graph, streams)
    assert none == 0 and all((x == y).all() for x, y in zip(on, off))
    assert st["keyswitches"] == st0["keyswitches"] and st["ntts"] == st0["ntts"]
