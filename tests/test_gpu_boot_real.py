"""GPU: the half bootstrap for real messages (ckks_boot.BootstrapEmitter(real_msg=True)) on the MI355X.  No new kernel and no new key: the
VM, the plan and the key-switch / NTT kernels run the half program as they run any other, so the check is the strongest one there is --
  * a whole half bootstrap at N = 2^12 (the smallest ring at which all three matrix groups have giant steps): final ciphertext limbs
    bit-identical to the oracle VM's on the same keys, plaintext and input limbs, in the plan and in the one-instruction-at-a-time loop,
    on 60-bit and mixed chains, with and without lazy sums;
  * at the reference's ring (N = 2^15, sparse secret): 1 prime -> 3 primes, scale exactly 2^40, the full form's own precision bound, and
    at most 0.55 x the full form's key switches counted by the VM itself;
  * every VM here holds the rotation keys of the FULL program only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_helpers import _get_ct, _import_keys, _mirror_vm  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402


def _program(logN, real_msg, target=3, r=5, ks=1, primes=None):
    """(K, cst, hevm, rotation offsets) of `one ciphertext at 1 prime, scale 2^40 -> bootstrap -> output` (tests/test_gpu_boot.py's helper,
    with the form as a parameter)"""
    from dacapo_amd import ckks_boot as cb
    from dacapo_amd import hevm_asm as ha

    K = target + cb.boot_levels(r) + ks
    b = ha.Builder(slots=1 << (logN - 1), init_level=1, shadow=False)
    x = b.input(None, level=1, scale_bits=40)
    em = cb.BootstrapEmitter(b, logN, K, target, r=r, ks=ks, primes=primes, real_msg=real_msg)
    y, _ = em.bootstrap(x, 2.0**40)
    b.output(y)
    cst, hv, info = b.assemble()
    return K, cst, hv, cb.rotation_offsets(hv)


def _vm(logN, K, weight, offs, opts=None, ks=1, primes=None):
    from dacapo_amd import runner

    hevm = runner.HEVM(seed=21, logN=logN, num_primes=K, vm_options=dict(opts or {}, secret_hw=weight), ks_special=ks, primes=primes)
    if offs:
        hevm.addRotationKeys(offs)
    return hevm


@pytest.mark.parametrize("plan,chain,ks,lazy", [(1, "60", 1, 0), (0, "60", 1, 0), (1, "mixed", 3, 0), (1, "mixed", 3, 1)])
def test_half_bootstrap_limbs_bit_identical_to_the_oracle(tmp_path, plan, chain, ks, lazy):
    """the method of test_bootstrap_limbs_bit_identical_to_the_oracle: keys imported from the VM, plaintext limbs mirrored, input limbs
    copied; lazy = 1: the oracle VM replays the plan's lazy sums (hevm_plan_lazy_groups)"""
    from dacapo_amd import ckks_boot as cb
    from dacapo_amd import lowlevel as ll

    logN = 12
    primes = None
    if chain == "mixed":
        K0 = 3 + cb.boot_levels() + ks
        primes = cb.mixed_prime_chain(logN, [60] + [51] * (K0 - 1 - ks) + [60] * ks)
    K, cst, hv, offs = _program(logN, True, ks=ks, primes=primes)
    _, _, _, offs_full = _program(logN, False, ks=ks, primes=primes)
    assert set(offs) <= set(offs_full)
    hevm = _vm(logN, K, 32, offs_full, {"plan": plan, "hyb_lazy_sum": lazy}, ks=ks, primes=primes)   # the full form's keys, nothing else
    o = Oracle(logN, K, primes=primes)
    if ks > 1:
        o.set_hybrid(ks)
    assert o.primes == (primes or cb.seal_prime_chain(logN, K))
    _import_keys(o, hevm, ll)
    D = o.dnum if ks > 1 else K - 1
    for step in offs:
        elt = o.elt_from_step(step)
        o.galois[elt] = ll.read_device(hevm.lw.hevm_galois_key(hevm.vm, elt), (D, 2, K, o.N))
    hevm.load_mem(cst, hv)
    ovm = _mirror_vm(hevm, ll, o, cst, hv, tmp_path)
    msg = np.random.default_rng(8).uniform(-1, 1, o.slots)
    hevm.setInput(0, msg)
    ovm.ciphers[0] = _get_ct(hevm, ll, 0)
    hevm.run()
    if lazy:
        groups = hevm.lazy_groups()
        print(f"lazy sums: {len(groups)} groups, {sum(len(g) for g in groups)} rotations")
        # six matrix products (three per transform, one chain each), every one with giant steps at this ring: half of the full form's
        # `>= 4 groups, >= 12 rotations`
        assert len(groups) >= 2 and sum(len(g) for g in groups) >= 6, groups
        ovm.set_lazy_groups(groups)
    ovm.run()
    r = ovm.prog.res_dst[0]
    got, want = _get_ct(hevm, ll, r), ovm.ciphers[r]
    assert got.ell == want.ell == 3 and got.scale == want.scale == 2.0**40
    assert (got.data == want.data).all()
    out = hevm.getOutput()[0]
    print(f"plan {plan}, chain {chain}, ks {ks}, lazy {lazy}: decrypted max error {np.abs(out - msg).max():.3e}")
    assert np.abs(out - msg).max() < 1e-5
    hevm.close()


def test_half_bootstrap_at_the_reference_ring_and_its_key_switch_count():
    """N = 2^15, weight 64: test_bootstrap_at_the_reference_ring_restores_levels_and_message's own bound (the full form measures 7e-8 /
    1.5e-8).  The VM is created with the FULL program's rotation keys only; it then runs the full program too, and the VM's own count of
    key switches must drop to at most 0.55 x."""
    logN = 15
    K, cst, hv, offs = _program(logN, True)
    _, cstf, hvf, offs_full = _program(logN, False)
    assert set(offs) <= set(offs_full)
    hevm = _vm(logN, K, 64, offs_full)
    hevm.load_mem(cst, hv)
    msg = np.random.default_rng(3).uniform(-1, 1, hevm.slots)
    hevm.setInput(0, msg)
    assert hevm.getCtxt(0).level == 1
    hevm.run()
    c = hevm.getCtxt(hevm.getResIdx(0))
    assert c.level == 3 and c.scale == 2.0**40
    err = np.abs(hevm.getOutput()[0] - msg)
    ks_half = hevm.stats()["keyswitches"]
    print(f"half: max error {err.max():.3e}, rms {np.sqrt(np.mean(err**2)):.3e}, {ks_half} key switches")
    assert err.max() < 1e-6 and np.sqrt(np.mean(err**2)) < 1e-7
    hevm.load_mem(cstf, hvf)
    hevm.setInput(0, msg)
    hevm.run()
    errf = np.abs(hevm.getOutput()[0] - msg)
    ks_full = hevm.stats()["keyswitches"]
    print(f"full: max error {errf.max():.3e}, rms {np.sqrt(np.mean(errf**2)):.3e}, {ks_full} key switches; ratio {ks_half / ks_full:.3f}")
    assert errf.max() < 1e-6
    assert ks_half <= 0.55 * ks_full
    hevm.close()


def test_half_bootstrap_needs_no_new_key():
    """a VM that holds exactly the full program's rotation keys (and the default set every VM has) runs the half program"""
    logN = 12
    K, cst, hv, offs = _program(logN, True)
    _, _, _, offs_full = _program(logN, False)
    assert set(offs) <= set(offs_full)
    hevm = _vm(logN, K, 32, offs_full)
    hevm.load_mem(cst, hv)
    msg = np.random.default_rng(5).uniform(-1, 1, hevm.slots)
    hevm.setInput(0, msg)
    hevm.run()
    c = hevm.getCtxt(hevm.getResIdx(0))
    assert c.level == 3 and c.scale == 2.0**40
    assert np.abs(hevm.getOutput()[0] - msg).max() < 1e-5
    # every rotation found its direct key: one key switch per rotate / mulcc / conj instruction, none composed from hops
    from dacapo_amd import hevm_asm as ha

    opcodes = ha.unpack_hevm(hv)["ops"][:, 0]
    assert hevm.stats()["keyswitches"] == int(np.isin(opcodes, [ha.OP_ROTATE, ha.OP_MULCC, ha.OP_CONJ]).sum()) == 68
    hevm.close()
