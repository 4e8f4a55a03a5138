"""GPU: sparse-secret encapsulation (option boot_secret_hw, opcode 20 = hevm_asm.OP_KEYSWITCH).
  * the two switching keys: swk_down (s -> s') holds q0 and the special primes only; opcode 20 at level 1 (swk_down) and at the top level
    (swk_up) equals the oracle's key switch on the same key limbs, in the one-instruction loop and in the plan (graph), with SEAL's one-prime
    digits and with config 4's grouped digits (8 primes per digit, 9 special primes);
  * ModRaise under a DENSE main secret: wrapped in KEYSWITCH 0 / KEYSWITCH 1 its overflow I is as narrow as the ephemeral secret makes it;
  * a whole bootstrap at N = 2^15 under a dense main secret decrypts to the message, plan and loop bit-identical;
  * key directories: create_context writes both switching keys (boot_swk.seal + boot.txt, never the ephemeral secret); full and server VMs
    load them, a client VM does not, and the server bootstraps to the full VM's limbs;
  * config 4 under a weight-192 main secret + SSE(32): logits within 6e-4 of torch, wall time within 3 % of today's weight-64 run."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_helpers import _get_ct, _import_keys  # noqa: E402
from oracle.oracle import Ciphertext, Oracle  # noqa: E402


def _vm(logN, K, main_hw, boot_hw, opts=None, ks=1, alpha=None, seed=23):
    from dacapo_amd import runner

    return runner.HEVM(seed=seed, logN=logN, num_primes=K, ks_special=ks, ks_alpha=alpha,
                       vm_options=dict(opts or {}, secret_hw=main_hw, boot_secret_hw=boot_hw))


def _switch_keys(hevm, ll, K, N, ks, digits):
    import ctypes

    down, up, limbs = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
    assert hevm.lw.hevm_boot_switch_keys(hevm.vm, ctypes.byref(down), ctypes.byref(up), ctypes.byref(limbs)) == 1
    assert limbs.value == 1 + ks
    # what the VM actually holds (hevm_key_buffers: the buffers the replicas broadcast and the digest covers): the down key is
    # [1][2][1 + ks][N] -- q0 and the special primes, nothing else -- and the up key one full-chain key
    held = dict(hevm.keyBuffers())
    assert held[down.value] == 2 * (1 + ks) * N
    assert held[up.value] == digits * 2 * K * N
    kd = ll.read_device(down.value, (1, 2, limbs.value, N))
    ku = ll.read_device(up.value, (digits, 2, K, N))
    return kd, ku


@pytest.mark.parametrize("geometry", ["seal", "grouped"])
@pytest.mark.parametrize("plan", [0, 1])
def test_keyswitch_opcode_bit_exact_against_the_oracle(geometry, plan):
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import lowlevel as ll

    logN = 12
    if geometry == "seal":
        K, ks, alpha = 6, 1, 1
    else:
        K, ks, alpha = 4 * 8 + 9, 9, 8                                       # config 4's key shape: 4 digits of 8 primes, 9 special primes
    hevm = _vm(logN, K, 0, 32, {"plan": plan}, ks=ks, alpha=alpha)
    o = Oracle(logN, K)
    if ks > 1:
        o.set_hybrid(ks, alpha)
    N, top = o.N, K - ks
    D = o.dnum if ks > 1 else K - 1
    _import_keys(o, hevm, ll, elts=[])
    kd, ku = _switch_keys(hevm, ll, K, N, ks, D)
    # the down key in the full layout for the oracle: digit 0 at q0 and the special primes (what a level-1 key switch reads); zeros elsewhere
    full_down = np.zeros((D, 2, K, N), dtype=np.uint64)
    full_down[0, :, 0] = kd[0, :, 0]
    full_down[0, :, K - ks:] = kd[0, :, 1:]
    KS = ha.OP_KEYSWITCH
    ops = [(KS, 2, 0, 0),                                                    # r2 = r0 (1 prime) switched s -> s'
           (KS, 3, 1, 1)]                                                    # r3 = r1 (top level) switched s' -> s
    hv = ha.pack_hevm([40, 40], [1, top], [40, 40], [1, top], [2, 3], 4, 0, top, np.array(ops, dtype=np.uint16))
    hevm.load_mem(ha.pack_cst([np.zeros(1)]), hv)
    rng = np.random.default_rng(6)
    m0, m1 = rng.uniform(-1, 1, o.slots), rng.uniform(-1, 1, o.slots)
    hevm.setInput(0, m0)
    hevm.setInput(1, m1)
    x0, x1 = _get_ct(hevm, ll, 0), _get_ct(hevm, ll, 1)
    hevm.run()
    got_down, got_up = _get_ct(hevm, ll, 2), _get_ct(hevm, ll, 3)
    o.galois = {1: full_down}
    want_down = o.apply_galois(x0, 1)
    o.galois = {1: np.ascontiguousarray(ku)}
    want_up = o.apply_galois(x1, 1)
    assert got_down.ell == 1 and got_up.ell == top and got_down.scale == got_up.scale == 2.0**40
    assert (got_down.data == want_down.data).all()
    assert (got_up.data == want_up.data).all()
    hevm.close()


def _centered_crt2(o, ct):
    """decryption of the first two limbs under the oracle's (main) secret, as centered integers mod q0 q1 (coefficient form)"""
    q0, q1 = int(o.primes[0]), int(o.primes[1])
    two = Ciphertext(np.ascontiguousarray(ct.data[:, :2]), ct.scale)
    t = o.ntt_inv(o.decrypt(two).data, [0, 1])
    a, b = t[0].astype(object), t[1].astype(object)
    inv = pow(q0, -1, q1)
    x = a + q0 * (((b - a) % q1) * inv % q1)
    Q = q0 * q1
    return np.where(x > Q // 2, x - Q, x), q0


def test_modraise_overflow_under_a_dense_secret_stays_narrow_with_sse():
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import lowlevel as ll

    logN, K = 15, 6
    top = K - 1
    hevm = _vm(logN, K, 0, 32, {"plan": 1})
    o = Oracle(logN, K)
    _import_keys(o, hevm, ll, elts=[])
    s = o.ntt_inv(o.sk, [0])[0]
    assert int((s != 0).sum()) > o.N // 2                                   # the main secret is dense (uniform ternary)
    KS, MR = ha.OP_KEYSWITCH, ha.OP_MODRAISE
    ops = [(KS, 1, 0, 0), (MR, 2, 1, top), (KS, 3, 2, 1),                   # SSE: s -> s', ModRaise, s' -> s
           (MR, 4, 0, top)]                                                  # without: ModRaise under the dense secret itself
    hv = ha.pack_hevm([40], [1], [40, 40], [top, top], [3, 4], 5, 0, 1, np.array(ops, dtype=np.uint16))
    hevm.load_mem(ha.pack_cst([np.zeros(1)]), hv)
    hevm.setInput(0, np.random.default_rng(7).uniform(-1, 1, o.slots))
    hevm.run()
    widths = {}
    for name, r in (("sse", 3), ("dense", 4)):
        t, q0 = _centered_crt2(o, _get_ct(hevm, ll, r))
        I = np.array([int((v + q0 // 2) // q0) for v in t], dtype=np.int64)   # |message + noise| << q0 / 2: the quotient is I
        widths[name] = (int(np.abs(I).max()), float(I.std()))
    print("ModRaise overflow I, max |I| / sigma:", widths)
    assert widths["sse"][0] <= 12
    assert widths["dense"][0] > 40                                           # what SSE avoids: sigma ~ sqrt((2N/3 + 1) / 12) ~ 43
    hevm.close()


def test_one_bootstrap_under_a_dense_secret_with_sse():
    from dacapo_amd import ckks_boot as cb
    from dacapo_amd import lowlevel as ll

    logN = 15
    K, cst, hv, offs, _ = cb.single_bootstrap_program(logN, sse=True)
    msg = np.random.default_rng(3).uniform(-1, 1, 1 << (logN - 1))
    outs, limbs = [], []
    for plan in (1, 0):
        hevm = _vm(logN, K, 0, 32, {"plan": plan}, seed=41)
        hevm.addRotationKeys(offs)
        hevm.load_mem(cst, hv)
        hevm.setInput(0, msg)
        limbs.append(_get_ct(hevm, ll, 0).data.copy())
        hevm.run()
        r = hevm.getResIdx(0)
        c = _get_ct(hevm, ll, r)
        assert c.ell == 3 and c.scale == 2.0**40
        limbs.append(c.data.copy())
        outs.append(hevm.getOutput()[0])
        hevm.close()
    assert (limbs[0] == limbs[2]).all()                                      # same seed: the same input ciphertext in both VMs
    assert (limbs[1] == limbs[3]).all()                                      # plan + graph == the one-instruction loop, limb for limb
    err = np.abs(outs[0] - msg)
    print(f"bootstrap under a dense secret + SSE(32): max error {err.max():.3e}, rms {np.sqrt(np.mean(err**2)):.3e}")
    assert err.max() < 1e-3


def test_key_directory_round_trip_carries_the_switching_keys(tmp_path):
    """create_context with boot_secret_hw writes boot_swk.seal (SEAL's KSwitchKeys container: s -> s' over 1 + ks_special limbs, s' -> s over
    the chain) and boot.txt; initFullVM / initServerVM load both keys, initClientVM does not; a server VM bootstraps (default Galois keys,
    NAF hops) to exactly the full VM's limbs"""
    import ctypes

    from dacapo_amd import ckks_boot as cb
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    logN, ks = 12, 3
    K, cst, hv, _, _ = cb.single_bootstrap_program(logN, ks=ks, sse=True)
    N = 1 << logN
    with runner.options(logn=logN, primes=K, ks_special=ks, secret_hw=0, boot_secret_hw=32):
        runner.lw.create_context(str(tmp_path).encode())
    assert sorted(os.listdir(tmp_path)) == sorted(["parm.seal", "pub.seal", "sec.seal", "relin.seal", "gal.seal", "hybrid.txt", "boot.txt",
                                                   "boot_swk.seal"])                # no file for the ephemeral secret
    assert (tmp_path / "boot.txt").read_text().startswith("boot_secret_hw=32")

    def switch_keys(vm):
        down, up, limbs = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
        ok = vm.lw.hevm_boot_switch_keys(vm.vm, ctypes.byref(down), ctypes.byref(up), ctypes.byref(limbs))
        if not ok:
            return None
        D = (K - ks + ks - 1) // ks
        return ll.read_device(down.value, (1, 2, limbs.value, N)), ll.read_device(up.value, (D, 2, K, N))

    client = runner.HEVM(path=str(tmp_path), option="client")
    assert switch_keys(client) is None                                        # evaluation keys: not a client's
    client.close()
    full = runner.HEVM(path=str(tmp_path), option="full")
    server = runner.HEVM(path=str(tmp_path), option="server")
    kf, ksv = switch_keys(full), switch_keys(server)
    assert kf[0].shape == (1, 2, 1 + ks, N)
    assert all((a == b).all() for a, b in zip(kf, ksv))
    msg = np.random.default_rng(12).uniform(-1, 1, N // 2)
    res = []
    for vm in (full, server):
        vm.load_mem(cst, hv)
        if vm is full:
            vm.setInput(0, msg)
            vm.saveCtxt(0, tmp_path / "arg0.ct")
        else:
            vm.loadCtxt(0, tmp_path / "arg0.ct")
        vm.run()
        res.append(_get_ct(vm, ll, vm.getResIdx(0)))
    assert res[0].ell == res[1].ell == 3 and res[0].scale == res[1].scale
    assert (res[0].data == res[1].data).all()                                 # the server bootstraps to the full VM's limbs
    err = np.abs(full.getOutput()[0] - msg)
    print(f"N = 2^12, dense secret + SSE(32), default Galois keys: bootstrap max error {err.max():.3e}")
    assert err.max() < 1e-3
    full.close()
    server.close()


def _config4(*extra):
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "tools" / "legs" / "resnet_real_boot.py"), "1", "resnet20_nt16", "17", "1", "b14", "9", "8",
                        *extra], capture_output=True, text=True, timeout=900, cwd=str(root))
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_config4_with_a_weight_192_secret_and_sse():
    base = _config4()
    sse = _config4("--sse", "192:32")
    print(f"config 4: h = 64 {base['run_s']:.3f} s rms {base['rms_vs_torch']:.2e}; h = 192 + SSE(32) {sse['run_s']:.3f} s "
          f"rms {sse['rms_vs_torch']:.2e}")
    assert sse["real_bootstraps"] == base["real_bootstraps"] == 38
    assert sse["key_switches"] == base["key_switches"] + 2 * 38
    assert sse["rms_vs_torch"] <= 6e-4
    assert sse["run_s"] <= 1.03 * base["run_s"]
