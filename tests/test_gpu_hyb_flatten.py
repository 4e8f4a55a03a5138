"""Flattened rotate-and-add stages under grouped-digit keys (csrc/hybrid_ks.hip hyb_mac_stage_kernel, hybrid_fused.hip hybf_rotate_stages,
dc_ct_rotate_stage_add; option hyb_flatten_sums, plan_exec.hip section 1a).  The reference is the oracle with the context's (ks_special, ks_alpha):
orc_rotate_acc_hybrid per member, the accumulators added limb-wise, one orc_moddown_hybrid onto (sum_k galois_k(c0), 0), Oracle.add: == on every limb."""
import ctypes
import dataclasses
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from gpu_helpers import _get_ct, _import_keys, _mirror_vm
from oracle.oracle import Ciphertext, LazySum, Oracle, _p, splitmix_fill
from test_gpu_ks_flatten import _ReplayVM
from test_gpu_prime_widths import _chain

pytestmark = pytest.mark.gpu
ROOT, LOGN, N = Path(__file__).resolve().parent.parent, 12, 1 << 12


class StageOracle(Oracle):
    def member(self, x, elt):
        """Oracle.rotate_lazy's last hop, named by its element"""
        acc = np.zeros((2, x.ell + self.ks, self.N), dtype=np.uint64)
        self.L.orc_rotate_acc_hybrid(self.ctx, x.ell, _p(np.ascontiguousarray(x.data[1])), ctypes.c_uint32(elt), _p(self.galois[elt]), _p(acc))
        c0 = self.galois_ntt(x.data[0], elt)
        return LazySum(Ciphertext(np.stack([c0, np.zeros_like(c0)]), x.scale), acc, 0, 1, 1 << 30)

    def prefixes(self, x, elts):
        """the finished sum (one orc_moddown_hybrid) after each member"""
        s, zero = None, Ciphertext(np.zeros_like(x.data), x.scale)
        for e in elts:
            s = self.member(x, e) if s is None else self.lazy_add(s, self.member(x, e))
            yield self.lazy_add(dataclasses.replace(s, size=s.have, acc=s.acc.copy()), zero)  # (the mod-down works in place)

    def rotate_sum(self, members, ell):  # (the method _ReplayVM asks for)
        return list(self.prefixes(members[0][0], [m[1] for m in members]))[-1]


@functools.lru_cache(maxsize=None)
def _env(K, bits=60):
    """oracle with the keys of the offsets 1 .. 63, those keys on the device, a context; per level the operands and the prefix sums, made once"""
    from dacapo_amd import lowlevel as ll

    primes = _chain(LOGN, [bits] * K) if bits != 60 else None
    o = StageOracle(LOGN, K, primes=primes)
    o.set_hybrid(2, 2)
    elts = [o.elt_from_step(s) for s in range(1, 64)]
    o.keygen(seed=0x4845564D, galois_elts=elts, relin=False)
    ctx = ll.Context(LOGN, K, primes=primes, special=2, alpha=2)
    assert ctx.primes == o.primes and ctx.key_digits == o.dnum
    edge = np.broadcast_to(np.array(o.primes, dtype=np.uint64)[None, None, :, None] - np.uint64(1), o.galois[elts[0]].shape).copy()
    return o, elts, ctx, {e: ll.DeviceBuffer.from_host(o.galois[e]) for e in elts}, edge, ll.DeviceBuffer.from_host(edge)


@functools.lru_cache(maxsize=None)
def _level(K, ell, edge=False, bits=60, upto=63):
    """source, addend and, per count, Oracle.add(addend, the stage's sum) and the bare sum; edge: q - 1 everywhere, keys included"""
    o, elts = _env(K, bits)[:2]
    q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
    x, y = (np.stack([np.stack([splitmix_fill(s + 7 * p + i + 100 * ell, N) for i in range(ell)]) % q for p in range(2)]) for s in (51, 61))
    keys = o.galois
    if edge:
        x[:], y[:], o.galois = q - np.uint64(1), q - np.uint64(1), dict.fromkeys(elts, _env(K, bits)[4])
    sums = list(o.prefixes(Ciphertext(x, 2.0**40), elts[:upto]))
    o.galois = keys
    return x, y, [o.add(Ciphertext(y, 2.0**40), s).data for s in sums], [s.data for s in sums]


def _call(K, ell, count, x, y, edge=False, bits=60, dst="new", addend="y"):
    """dc_ct_rotate_stage_add -> (the result, the source and the addend read back)"""
    from dacapo_amd import lowlevel as ll

    _, elts, ctx, dkeys, _, dedge = _env(K, bits)
    dx, dy = ll.DeviceBuffer.from_host(x), ll.DeviceBuffer.from_host(y)
    dd = {"new": ll.DeviceBuffer((2, ell, N)), "x": dx, "y": dy}[dst]
    ctx.rotate_stage_add(dd, ell * N, {"y": dy, "x": dx, None: None}[addend], ell * N, dx, ell * N, elts[:count],
                         [dedge if edge else dkeys[e] for e in elts[:count]], ell)
    ctx.sync()
    return dd.to_host(), dx.to_host(), dy.to_host()


# one partial digit; one full; full + partial; two full + partial -- and both sides of the kernel's reduce interval floor(16 / G) at the level's G
@pytest.mark.parametrize("K,ell,counts", [(6, 1, (1, 3, 7, 16, 17, 63)), (6, 2, (1, 3, 7, 16, 17, 63)), (6, 3, (1, 3, 7, 8, 9, 63)), (7, 5, (1, 3, 7, 5, 6, 63))])
@pytest.mark.parametrize("which", [0, 1, 2, 3, 4, 5, "edge"])
def test_stage_equals_the_oracle_composition(K, ell, counts, which):
    edge = which == "edge"
    count = 63 if edge else counts[which]
    x, y, want, _ = _level(K, ell, edge)
    got, x_after, y_after = _call(K, ell, count, x, y, edge)
    assert (got == want[count - 1]).all() and (x_after == x).all() and (y_after == y).all()


# both fused sequences (hyb_fuse = 2 differs from 1 from four primes up) and the generic-width build on a 51-bit chain
@pytest.mark.parametrize("K,ell,fuse,bits", [(6, 3, 1, 60), (7, 5, 2, 60), (6, 3, 2, 51)])
@pytest.mark.parametrize("dst,addend", [("new", "y"), ("new", "x"), ("y", "y"), ("x", "y"), ("new", None)])
def test_addend_placement_in_both_sequences_and_builds(K, ell, fuse, bits, dst, addend):
    from dacapo_amd import runner

    x, y, with_y, bare = _level(K, ell, False, bits, 3)
    with runner.options(hyb_fuse=fuse):
        got, x_after, y_after = _call(K, ell, 3, x, y, False, bits, dst, addend)
    want = {"y": with_y[2], "x": _env(K, bits)[0].add(Ciphertext(x, 1.0), Ciphertext(bare[2], 1.0)).data, None: bare[2]}[addend]
    assert (got == want).all() and (dst == "x" or (x_after == x).all()) and (dst == "y" or (y_after == y).all())


@pytest.mark.parametrize("graph,streams,f", [(0, 1, 3), (1, 1, 3), (2, 1, 3), (1, 2, 3), (1, 1, 0)])
def test_program_equals_the_replay_of_the_exported_groups(graph, streams, f, tmp_path):
    """chains of 2, 3 and 5 hops over one source; near-misses: a stage result read three times, a program result inside a chain, a plain lazy sum"""
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    K, rng = 6, np.random.default_rng(61)
    b = ha.Builder(slots=N // 2, init_level=K - 2, policy="eager", shadow=True)
    x, w, v = (b.input(rng.uniform(-1, 1, N // 2)) for _ in range(3))
    ends, kept = [], []
    for offs in ([1, 2], [3, 6, 12], [5, 10, 20, 40, 80], [7, 14, 28], [9, 18, 36, 72]):
        y = x
        for o_ in offs:
            y = b.add(y, b.rotate(y, o_))
            kept.append(y)
        ends.append(y)
    outs = ends + [b.add(kept[10], w), kept[14], b.add(b.rotate(w, 4), b.rotate(v, 8))]  # x + rot(x, 7) has a third reader; [9, 18]'s end is a result
    for r in outs:
        b.output(r)
    for _ in range(16):  # (recycle the registers: a rotation result that a register still names when the program ends stays observable)
        b.output(b.negate(ends[0]))
    cst, hv, _ = b.assemble()
    regs = [int(r) for r in ha.unpack_hevm(hv)["res_dst"]]
    hevm = runner.HEVM(seed=29, logN=LOGN, num_primes=K, ks_special=2, vm_options={"plan_graph": graph, "hyb_lazy_sum": 1, "hyb_flatten_sums": f})
    hevm.set_streams(streams)
    hevm.load_mem(cst, hv)
    added = hevm.flatten_offsets()
    assert bool(added) == bool(f)
    if added:
        hevm.addRotationKeys(added)
    for s in range(streams):
        hevm.select_stream(s)
        for i, a in enumerate(b.args):
            hevm.setInput(i, np.roll(a.plain, 5 * s))
    hevm.run()
    hevm.run()  # (a graph is replayed: the second run's limbs are the ones compared)
    groups, st = hevm.flatten_groups(), hevm.flatten_stats()
    o = StageOracle(LOGN, K)
    o.set_hybrid(2)
    _import_keys(o, hevm, ll, elts=o.default_galois_elts() + [o.elt_from_step(off) for off in added], relin=False)
    for s in range(streams):
        hevm.select_stream(s)
        ovm = _mirror_vm(hevm, ll, o, cst, hv, tmp_path)
        ovm.set_lazy_groups(hevm.lazy_groups())
        for i in range(len(b.args)):
            ovm.ciphers[i] = _get_ct(hevm, ll, i)
        _ReplayVM(ovm, groups if f else []).run()
        assert all((_get_ct(hevm, ll, r).data == ovm.ciphers[r].data).all() for r in regs), (graph, s)
    hops = sorted(len(g[1]) for g in groups) if f else []
    assert hops == ([2, 2, 2, 2, 2, 3, 3] if f else []) and len(hevm.lazy_groups()) == 1  # 2; 3; 3 + 2; 7 | 14, 28; 9, 18 | 36, 72
    assert st == {"groups": streams * len(hops), "members": streams * sum(2 ** h - 1 for h in hops), "hops_absorbed": streams * sum(hops)}
    hevm.close()


@pytest.mark.parametrize("code,words", [
    ("runner.HEVM(fresh=True, logN=12, num_primes=6, ks_special=2, vm_options={'hyb_flatten_sums': 3})", ["hyb_flatten_sums", "hyb_lazy_sum >= 1"]),
    ("runner.HEVM(fresh=True, logN=12, num_primes=4, vm_options={'hyb_flatten_sums': 3})", ["hyb_flatten_sums", "ks_flatten_sums"]),
    ("c = ll.Context(12, 4); d = ll.DeviceBuffer((2, 2, 4096)); c.rotate_stage_add(d, 8192, None, 0, d, 8192, [3], [d], 2)", ["dc_ct_rotate_sum_hoisted_add"])])
def test_refusals_name_what_is_missing(code, words):
    r = subprocess.run([sys.executable, "-c", f"from dacapo_amd import runner, lowlevel as ll\n{code}\nprint('went on')\n"], cwd=str(ROOT),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "went on" not in r.stdout and all(w in r.stderr for w in words), (r.returncode, r.stderr)
