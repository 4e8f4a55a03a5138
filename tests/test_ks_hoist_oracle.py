"""Hoisted rotations on SEAL-layout keys (option ks_hoist, dc_ct_rotate_hoisted; dacapo_amd/csrc/hoist_ks.hip), the parts that need no GPU:
  * the DEFINITION the GPU tests compare against -- oracle orc_rotate_ks_hybrid on a context left at one special prime and one prime per
    digit: the digits of c1 taken before the automorphism, the Galois permutation applied to the lifted digits in the NTT domain -- is a
    correct rotation (it decrypts to the rotated message) and is NOT Oracle.apply_galois (every limb differs), so a GPU test that compared
    against the wrong one of the two would fail;
  * the two new symbols are declared in the headers and exported by all four builds of the library."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle.oracle import Ciphertext, Oracle, _p

ROOT = Path(__file__).resolve().parent.parent


def hoisted_galois(o: Oracle, a: Ciphertext, elt: int) -> Ciphertext:
    """the hoisted hop on a SEAL-mode oracle: galois(c0) + KS of c1's digits read through the permutation"""
    assert (o.ks, o.alpha) == (1, 1)
    c0 = o.galois_ntt(a.data[0], elt)
    c1 = np.zeros_like(c0)
    key = o.galois[elt]
    assert key.shape == (o.K - 1, 2, o.K, o.N)
    o.L.orc_rotate_ks_hybrid(o.ctx, a.ell, _p(np.ascontiguousarray(a.data[1])), C.c_uint32(elt), _p(key), _p(c0), _p(c1))
    return Ciphertext(np.stack([c0, c1]), a.scale)


@pytest.mark.parametrize("logN,K", [(10, 5), (12, 4)])
def test_hoisted_hop_is_a_rotation_and_differs_from_seals_hop(logN, K):
    """every level, steps 1 / -3 / 5 and the conjugation, scale 2^40: max slot error < 1e-6 (SEAL's own hop: 7e-9 ... 3.5e-7 on the same
    inputs; the hoisted one was at most 4.2e-7 with this test's message and keys), and no limb equals SEAL's"""
    o = Oracle(logN, K)
    steps = [1, -3, 5, 0]  # elt_from_step(0) = 2N - 1: the conjugation
    elts = [o.elt_from_step(s) for s in steps]
    o.keygen(seed=0x4845564D, galois_elts=elts)
    slots = o.slots
    rng = np.random.default_rng(logN * 100 + K)
    v = rng.uniform(-1, 1, slots)
    worst = 0.0
    for ell in range(1, K):
        ct = o.encrypt(o.encode(v, 2.0**40, ell))
        for step, elt in zip(steps, elts):
            got = hoisted_galois(o, ct, elt)
            ref = o.apply_galois(ct, elt)
            want = np.roll(v, -step)  # the conjugate of a real vector is itself
            err = float(np.abs(o.decode(o.decrypt(got)).real[:slots] - want).max())
            worst = max(worst, err)
            print(f"N=2^{logN} K={K} ell={ell} step={step}: hoisted err {err:.2e}, SEAL hop err "
                  f"{float(np.abs(o.decode(o.decrypt(ref)).real[:slots] - want).max()):.2e}")
            assert err < 1e-6, (ell, step, err)
            assert got.data.shape == ref.data.shape
            if ell > 1:  # (at one prime there is no cross-prime lift: only the special prime's digit differs, c0 and c1 still do)
                assert (got.data != ref.data).reshape(2 * ell, -1).any(axis=1).all(), (ell, step)
            assert not (got.data == ref.data).all(), (ell, step)
    print("worst", worst)


@pytest.mark.parametrize("which", ["default", "generic_width", "default_hooks", "generic_width_hooks"])
def test_new_symbols_are_declared_and_exported(which):
    """dc_ct_rotate_hoisted / hevm_last_run_hoist_stats: in the headers, in csrc/exports.map, and in `nm -D` of every build"""
    import dacapo_amd as pkg

    new = {"dc_ct_rotate_hoisted": "dacapo_ckks.h", "hevm_last_run_hoist_stats": "hevm_abi.h"}
    path = {"default": pkg.LIB_PATH_RELEASE, "generic_width": pkg.LIB_PATH_GW_RELEASE,
            "default_hooks": pkg._LIB_DIR / "libSEAL_HEVM_hooks.so", "generic_width_hooks": pkg._LIB_DIR / "libSEAL_HEVM_gw_hooks.so"}[which]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    listed = set(re.findall(r"^\s+(\w+);", (ROOT / "dacapo_amd" / "csrc" / "exports.map").read_text(), flags=re.M))
    for name, header in new.items():
        text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
        assert re.search(r"\b" + name + r"\s*\(", text), (name, header)
        assert name in listed, name
        assert name in exported, (name, which)
