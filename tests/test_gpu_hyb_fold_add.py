"""Rotate-and-add under grouped-digit keys: the addend enters the data-prime accumulators as P . y (csrc/hybrid_ks.hip hyb_mac_kernel<3>;
hyb_prepare_rot_kernel under hyb_fuse = 0; option hyb_fold_add, csrc/plan_exec.hip section 3a).  Nothing is rounded: == on every limb."""
import numpy as np
import pytest

from gpu_helpers import _get_ct, _import_keys, _mirror_vm
from oracle.oracle import Ciphertext, Oracle, splitmix_fill

pytestmark = pytest.mark.gpu
LOGN, N = 12, 1 << 12
ELTS = (3, 2 * N - 1, 1)  # a rotation, the conjugation, the identity


@pytest.fixture(scope="module", params=[(7, 2, 2), (8, 3, 2)], ids=["K7_ks2_a2", "K8_ks3_a2"])
def env(request):
    K, ks, alpha = request.param
    o = Oracle(LOGN, K)
    o.set_hybrid(ks, alpha)
    o.keygen(seed=0x4845564D, galois_elts=list(ELTS), relin=False)
    return o, request.param, {}  # (the oracle's results per (level, key, edge): computed once for the three launch sequences)


@pytest.mark.parametrize("fuse", [1, 2, 0])
@pytest.mark.parametrize("ell", [1, 2, 3, 5])  # one partial digit; one full; full + partial (own-digit and raised operands mix); two full + partial
def test_rotate_hop_add_matches_rotate_then_add(env, ell, fuse):
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    o, (K, ks, alpha), cache = env
    L, st, q = ll.lib(), ell * N, np.array(o.primes[:ell], dtype=np.uint64)[:, None]
    with runner.options(hyb_fuse=fuse):
        ctx = ll.Context(LOGN, K, special=ks, alpha=alpha)
        assert ctx.primes == o.primes and ctx.key_digits == o.dnum
        for elt, edge in [(e, False) for e in ELTS] + [(3, True)] * (ell == 3):
            if (ell, elt, edge) not in cache:
                a, y = (np.stack([np.stack([splitmix_fill(s + 7 * p + i + 100 * ell, N) for i in range(ell)]) % q for p in range(2)]) for s in (51, 61))
                if edge:  # every limb of Y and of A.c0 at q - 1: the largest galois(c0) + y0 and products with P that must come back canonical
                    a[0], y[:] = q - np.uint64(1), q - np.uint64(1)
                rot = o.apply_galois(Ciphertext(a, 2.0**40), elt)
                cache[ell, elt, edge] = a, y, o.add(rot, Ciphertext(y, 2.0**40)).data, o.add(rot, Ciphertext(a, 2.0**40)).data
            a, y, want_other, want_self = cache[ell, elt, edge]
            da, dy, dd, dk = ll.DeviceBuffer.from_host(a), ll.DeviceBuffer.from_host(y), ll.DeviceBuffer((2, ell, N)), ll.DeviceBuffer.from_host(o.galois[elt])
            L.dc_ct_rotate_hop_add(ctx.h, dd.ptr, st, da.ptr, st, dy.ptr, st, elt, dk.ptr, ell, None)  # distinct from src and dst
            assert (dd.to_host() == want_other).all() and (da.to_host() == a).all() and (dy.to_host() == y).all(), ("another ciphertext", elt, edge)
            L.dc_ct_rotate_hop_add(ctx.h, dd.ptr, st, da.ptr, st, da.ptr, st, elt, dk.ptr, ell, None)  # the source: y' = y + rotate(y)
            assert (dd.to_host() == want_self).all(), ("the source", elt, edge)
            L.dc_ct_rotate_hop_add(ctx.h, dy.ptr, st, da.ptr, st, dy.ptr, st, elt, dk.ptr, ell, None)  # the destination
            assert (dy.to_host() == want_other).all(), ("the destination", elt, edge)


@pytest.mark.parametrize("graph,lazy", [(1, 0), (0, 0), (2, 0), (1, 1)])
def test_program_folds_and_keeps_every_limb(graph, lazy, tmp_path):
    """two three-stage chains over ONE source beside a bare rotation of it (one decomposition slot, items with and without an addend), and two
    near-misses: a rotation result read twice, a sum of two rotations of one wave (a lazy-sum group under hyb_lazy_sum = 1); two streams"""
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    K, ks, rng = 7, 2, np.random.default_rng(53)
    b = ha.Builder(slots=N // 2, init_level=K - ks, policy="eager", shadow=True)
    x, w, v = (b.input(rng.uniform(-1, 1, N // 2)) for _ in range(3))
    ya, yb = x, x
    for oa, ob in ((1, 2), (2, 4), (4, 8)):
        ya, yb = b.add(ya, b.rotate(ya, oa)), b.add(yb, b.rotate(yb, ob))
    twice = b.rotate(w, 1)
    for r in [ya, yb, b.rotate(x, 16), b.add(w, twice), b.add(twice, v), b.add(b.rotate(w, 4), b.rotate(v, 8))]:
        b.output(r)
    for _ in range(16):  # (recycle the registers: a rotation result that a register still names when the program ends stays observable)
        b.output(b.negate(ya))
    cst, hv, _ = b.assemble()
    regs, runs = [int(r) for r in ha.unpack_hevm(hv)["res_dst"]], {}
    for on in (0, 1):
        hevm = runner.HEVM(seed=29, logN=LOGN, num_primes=K, ks_special=ks, vm_options={"plan_graph": graph, "hyb_lazy_sum": lazy, "hyb_fold_add": on})
        hevm.set_streams(2)
        hevm.load_mem(cst, hv)
        for s in range(2):
            hevm.select_stream(s)
            for i, a in enumerate(b.args):
                hevm.setInput(i, np.roll(a.plain, 5 * s))
        hevm.run()
        hevm.run()  # (a graph is replayed: the second run's limbs are the ones compared)
        got = []
        for s in (1, 0):
            hevm.select_stream(s)
            got.append([_get_ct(hevm, ll, r) for r in regs])
        if not on:  # the oracle VM on stream 0's inputs, with the plan's lazy groups when it has some
            o = Oracle(LOGN, K)
            o.set_hybrid(ks)
            _import_keys(o, hevm, ll, relin=False)
            ovm = _mirror_vm(hevm, ll, o, cst, hv, tmp_path)
            if lazy:
                ovm.set_lazy_groups(hevm.lazy_groups())
            for i in range(len(b.args)):
                ovm.ciphers[i] = _get_ct(hevm, ll, i)
            ovm.run()
            assert all((c.data == ovm.ciphers[r].data).all() and c.scale == ovm.ciphers[r].scale for c, r in zip(got[1], regs)), "option off against the oracle VM"
        runs[on] = got, hevm.stats(), len(hevm.lazy_groups())
        hevm.close()
    print(f"add_folds off {runs[0][1]['add_folds']} on {runs[1][1]['add_folds']}; lazy groups {runs[0][2]} {runs[1][2]}")
    assert all((c.data == d.data).all() and c.scale == d.scale for s in range(2) for c, d in zip(runs[0][0][s], runs[1][0][s])), "option on against option off"
    assert runs[0][1]["add_folds"] == 0 and runs[1][1]["add_folds"] == 2 * 6  # 6 per stream: two chains of three stages
    assert runs[0][2] == runs[1][2] == lazy and all(runs[0][1][k] == runs[1][1][k] for k in ("ntts", "keyswitches"))
