"""Lazy sums on SEAL-layout keys (option ks_lazy_sum, dc_ct_rotate_sum_hoisted; dacapo_amd/csrc/hoist_ks.hip f_ks_gsum_kernel), the parts that
need no GPU:
  * the DEFINITION the GPU tests compare against -- per member oracle orc_rotate_acc_hybrid on a context left at one special prime and one prime
    per digit, Oracle.lazy_mul_plain / lazy_add, one orc_moddown_hybrid per sum -- is the hoisted hop when the sum has one member, is NOT the
    sum of hops when it has three (one rounding instead of three: a centred difference of at most 2 per coefficient), and decrypts to the
    expected slots, bare and times plaintexts;
  * the new entry point is declared and exported by all four builds, and the option exists with default 0."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle.oracle import Ciphertext, LazySum, Oracle, _p

ROOT = Path(__file__).resolve().parent.parent


class LazyOracle(Oracle):
    """a SEAL-mode oracle (one special prime, one prime per digit) whose hop is the hoisted definition (tests/test_gpu_ks_hoist.py HoistOracle)
    and whose rotate_lazy is Oracle.rotate_lazy's own body without the grouped-digit assertion: acc is [2][l + 1][N]"""

    def apply_galois(self, a: Ciphertext, elt: int) -> Ciphertext:
        assert (self.ks, self.alpha) == (1, 1)
        c0 = self.galois_ntt(a.data[0], elt)
        c1 = np.zeros_like(c0)
        key = self.galois[elt]
        assert key.shape == (self.K - 1, 2, self.K, self.N)
        self.L.orc_rotate_ks_hybrid(self.ctx, a.ell, _p(np.ascontiguousarray(a.data[1])), C.c_uint32(elt), _p(key), _p(c0), _p(c1))
        return Ciphertext(np.stack([c0, c1]), a.scale)

    def rotate_lazy(self, a: Ciphertext, steps: int, group: int, size: int) -> LazySum:
        hops = self.rotate_hops(steps)
        assert hops, "a rotation by zero has no key switch to share"
        for e in hops[:-1]:
            a = self.apply_galois(a, e)
        return self.galois_lazy(a, hops[-1], group, size)

    def galois_lazy(self, a: Ciphertext, elt: int, group: int = 0, size: int = 1) -> LazySum:
        """one hop by its Galois element, left in the raised basis"""
        assert (self.ks, self.alpha) == (1, 1)
        c0 = self.galois_ntt(a.data[0], elt)
        acc = np.zeros((2, a.ell + self.ks, self.N), dtype=np.uint64)
        self.L.orc_rotate_acc_hybrid(self.ctx, a.ell, _p(np.ascontiguousarray(a.data[1])), C.c_uint32(elt), _p(self.galois[elt]), _p(acc))
        return LazySum(Ciphertext(np.stack([c0, np.zeros_like(c0)]), a.scale), acc, group, 1, size)

    def lazy_finish(self, s: LazySum) -> Ciphertext:
        """the one division by P (what lazy_add does when the group's last member has joined)"""
        c0, c1 = s.base.data[0].copy(), s.base.data[1].copy()
        self.L.orc_moddown_hybrid(self.ctx, s.ell, _p(np.ascontiguousarray(s.acc)), _p(c0), _p(c1))
        return Ciphertext(np.stack([c0, c1]), s.base.scale)

    def rotate_sum(self, members, ell):
        """sum_k [pt_k] galois_{elt_k}(ct_k) with one division by P.  members: (ciphertext, element, plaintext or None, special limb [1][N] or None)"""
        total = None
        for ct, elt, pt, sp in members:
            t = self.galois_lazy(ct, elt, 0, len(members))
            if pt is not None:
                t = self.lazy_mul_plain(t, pt, sp)
            if total is None:
                total = t
            else:
                total.scale = t.scale
                total = self.lazy_add(total, t)
        return self.lazy_finish(total) if isinstance(total, LazySum) else total


def centred_coefficients(o, a, b):
    """(a - b) limb by limb, as centred coefficients (inverse NTT per limb); a, b: [2][l][N] NTT form"""
    ell = a.shape[1]
    out = []
    for p in range(2):
        q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
        d = (a[p] + (q - b[p])) % q
        c = o.ntt_inv(d, list(range(ell))).astype(object)
        qo = np.array(o.primes[:ell], dtype=object)[:, None]
        out.append(np.where(c > qo // 2, c - qo, c))
    return np.stack(out)


def test_lazy_sum_definition_on_seal_layout_keys():
    """N = 2^10, K = 5, l = 3 (section (a) of the issue's check list)"""
    logN, K, ell = 10, 5, 3
    o = LazyOracle(logN, K)
    steps = [1, -3, 5]
    elts = [o.elt_from_step(s) for s in steps]
    o.keygen(seed=0x4845564D, galois_elts=elts, relin=False)
    slots = o.slots
    rng = np.random.default_rng(5)
    vs = [rng.uniform(-1, 1, slots) for _ in steps]
    cts = [o.encrypt(o.encode(v, 2.0**40, ell)) for v in vs]
    # a group of one is the hoisted hop
    for ct, elt in zip(cts, elts):
        assert (o.rotate_sum([(ct, elt, None, None)], ell).data == o.apply_galois(ct, elt).data).all()
    # a bare sum of three: one rounding instead of three
    lazy = o.rotate_sum([(ct, elt, None, None) for ct, elt in zip(cts, elts)], ell)
    eager = o.add(o.add(o.apply_galois(cts[0], elts[0]), o.apply_galois(cts[1], elts[1])), o.apply_galois(cts[2], elts[2]))
    assert (lazy.data != eager.data).any()
    d = centred_coefficients(o, lazy.data, eager.data)
    worst = int(np.abs(d).max())
    print("centred coefficient difference, lazy sum of three against three hops: max", worst)
    assert worst <= 2  # four roundings (three hops and the one lazy division) of at most 1/2 each
    assert all((d[:, 0] == d[:, i]).all() for i in range(1, ell))  # (the same small integer under every prime)
    want = sum(np.roll(v, -s) for v, s in zip(vs, steps))
    err = float(np.abs(o.decode(o.decrypt(lazy)).real[:slots] - want).max())
    print(f"bare lazy sum: max slot error {err:.2e}")
    assert err < 1e-6
    # the same sum times plaintexts: the special-prime limb comes from the encoding at all K primes
    ws = [rng.uniform(-1, 1, slots) for _ in steps]
    pts = [o.encode(w, 2.0**40, ell) for w in ws]
    sps = [o.encode(w, 2.0**40, K).data[K - 1 : K] for w in ws]
    for pt, w in zip(pts, ws):
        assert (o.encode(w, 2.0**40, K).data[:ell] == pt.data).all()  # (the same encoded polynomial, limb for limb)
    lazy_p = o.rotate_sum([(ct, elt, pt, sp) for ct, elt, pt, sp in zip(cts, elts, pts, sps)], ell)
    assert lazy_p.scale == 2.0**80
    want_p = sum(w * np.roll(v, -s) for v, s, w in zip(vs, steps, ws))
    err_p = float(np.abs(o.decode(o.decrypt(lazy_p)).real[:slots] - want_p).max())
    print(f"lazy sum with plaintexts: max slot error {err_p:.2e}")
    assert err_p < 1e-6


@pytest.mark.parametrize("which", ["default", "generic_width", "default_hooks", "generic_width_hooks"])
def test_rotate_sum_entry_is_declared_and_exported(which):
    """dc_ct_rotate_sum_hoisted: in include/dacapo_ckks.h, in csrc/exports.map, and in `nm -D` of every build"""
    import dacapo_amd as pkg

    name = "dc_ct_rotate_sum_hoisted"
    path = {"default": pkg.LIB_PATH_RELEASE, "generic_width": pkg.LIB_PATH_GW_RELEASE,
            "default_hooks": pkg._LIB_DIR / "libSEAL_HEVM_hooks.so", "generic_width_hooks": pkg._LIB_DIR / "libSEAL_HEVM_gw_hooks.so"}[which]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    listed = set(re.findall(r"^\s+(\w+);", (ROOT / "dacapo_amd" / "csrc" / "exports.map").read_text(), flags=re.M))
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dacapo_ckks.h").read_text(), flags=re.S)
    assert re.search(r"\b" + name + r"\s*\(", text)
    assert name in listed
    assert name in exported, which


def test_ks_lazy_sum_is_a_known_option_with_default_zero():
    """asked of the library in a child process (an unknown option name aborts), with no option environment"""
    import os

    import dacapo_amd as pkg

    code = ("import ctypes, sys\n"
            "L = ctypes.CDLL(sys.argv[1])\n"
            "L.hevm_get_option.restype = ctypes.c_longlong\n"
            "print('value', L.hevm_get_option(b'ks_lazy_sum'))\n")
    env = {k: v for k, v in os.environ.items() if k != "DACAPO_HEVM_OPTIONS"}
    r = subprocess.run([sys.executable, "-c", code, str(pkg.LIB_PATH_RELEASE)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert "value 0" in r.stdout.split("\n"), r.stdout
    table = (ROOT / "dacapo_amd" / "csrc" / "options.cpp").read_text()
    assert re.search(r'\{\s*"ks_lazy_sum",\s*0\s*\}', table)
