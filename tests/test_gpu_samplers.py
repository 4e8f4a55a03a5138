"""GPU: the device samplers, key generation, Encryptor::encrypt and the zero-encryptions of opcode 10 against the host reference of their
definition (tests/sampler_reference.py), on the hooks builds: a seeded VM's two ChaCha20 keys are known, every draw is addressed, so every
coefficient of every key and of every fresh ciphertext is predicted.  Every comparison is == on whole arrays; there is no tolerance here.
  * key generation on the 60-bit build (N = 2^13, 7 primes): secret, public, relinearisation and every default Galois key;
  * the same on a chain of five 46-bit primes at the bottom of the allowed window (generic-width build), where the uniform sampler's retry
    branch runs: the reference predicts the retried coefficients and the test requires at least 4 of them in what it compares;
  * grouped digits; sparse secrets and the c1 halves of both switching keys of sparse-secret encapsulation;
  * Encryptor::encrypt, limb for limb, across objects, epochs and levels;
  * opcode 10: the zero-encryptions of a run are the predicted ones at the run's epoch in every execution form (captured graph, one
    lane without graph, built graph, one-instruction loop), and differ from run to run -- a replayed graph included."""
import ctypes
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sampler_reference as sr  # noqa: E402
from gpu_helpers import _get_ct  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
SEED = 0x4845564D
# the smallest primes = 1 mod 2N (N = 2^12) with 2^46 - q < 2^28: each rejects a 46-bit draw with probability ~2^-18
NARROW = [0x3ffff001e001, 0x3ffff002a001, 0x3ffff0048001, 0x3ffff005e001, 0x3ffff009a001]
RETRIED_46 = 8   # retried coefficients the reference predicts in the relinearisation and Galois keys of that chain for SEED


# ---- one VM per parameter set, shared by the tests of this module (tests/conftest.py closes what is left at the module's end) -----------
def _setup(seed, logN, ks=1, alpha=None, primes=None, num_primes=0, vm_options=None):
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    hevm = runner.HEVM(seed=seed, logN=logN, num_primes=num_primes, primes=primes, ks_special=ks, ks_alpha=alpha, vm_options=vm_options)
    o = Oracle(logN, hevm.K, primes=primes)
    K, N, D = hevm.K, hevm.N, hevm.key_digits
    v = SimpleNamespace(hevm=hevm, ll=ll, o=o, K=K, N=N, D=D, L=hevm.max_level, ks=ks, alpha=alpha or ks, keys=sr.rng_keys_from_test_seed(seed),
                        encryptions=0, runs=0)     # Encryptor::encrypt calls and run() calls made on this VM so far: the next object / the epoch
    v.sk = ll.read_device(hevm.lw.hevm_secret_key(hevm.vm), (K, N))
    v.pk = ll.read_device(hevm.lw.hevm_public_key(hevm.vm), (2, K, N))
    return v


@pytest.fixture(scope="module")
def vm60():
    v = _setup(SEED, 13, num_primes=7)
    yield v
    v.hevm.close()


@pytest.fixture(scope="module")
def vm46():
    v = _setup(SEED, 12, primes=NARROW)
    yield v
    v.hevm.close()


@pytest.fixture(scope="module")
def vm_grouped():
    v = _setup(SEED + 1, 12, ks=2, alpha=2, num_primes=7)
    yield v
    v.hevm.close()


@pytest.fixture(scope="module")
def vm_sparse():
    v = _setup(SEED + 2, 12, num_primes=6, vm_options={"secret_hw": 32, "boot_secret_hw": 32})
    yield v
    v.hevm.close()


# ---- key generation ------------------------------------------------------------------------------------------------------------------------
def _all(v):
    return list(range(v.K))


def check_secret_and_public_key(v, secret):
    """sk is the lifted secret polynomial; pk = (-(a s + e), a) with a, e the reference's; returns the retried coefficients of a"""
    o, primes = v.o, v.o.primes
    assert (o.ntt_inv(v.sk, _all(v)) == sr.lift(secret, primes)).all()
    a, retries = sr.uniform_poly(v.keys["pub"], 0, primes, v.N, sr.RNG_PK_A)
    assert (v.pk[1] == a).all()
    e = o.poly_neg(o.poly_add(v.pk[0], o.poly_mul(v.pk[1], v.sk)))
    assert (o.ntt_inv(e, _all(v)) == sr.lift(sr.small_poly(v.keys["secret"], 0, v.N, sr.RNG_PK_E), primes)).all()
    return int((retries > 0).sum())


def check_kswitch_key(v, key, key_id, new_key):
    """every digit j of a key for `new_key` (NTT form) under v.sk: c1 = the reference's uniform residues at object key_id * 64 + j, and
    -(c0 + c1 s) + [limb in digit j's group] (P mod q) new_key = the reference's error there, on every limb.  Returns the retried coefficients."""
    o, primes, K, N, L = v.o, v.o.primes, v.K, v.N, v.L
    P = 1
    for q in primes[L:]:
        P *= q
    retried = 0
    for j in range(v.D):
        a, e, retries = sr.kswitch_digit(v.keys, key_id, j, primes, N)
        assert (key[j, 1] == a).all(), (key_id, j)
        assert int(retries.max()) <= 1                                      # (a second retry of one coefficient: probability ~2^-36 each)
        retried += int((retries > 0).sum())
        factor = np.zeros((K, N), dtype=np.uint64)
        for i in range(j * v.alpha, min((j + 1) * v.alpha, L)):              # SEAL layout: alpha = 1, the one limb j
            factor[i] = P % primes[i]
        got = o.poly_add(o.poly_neg(o.poly_add(key[j, 0], o.poly_mul(key[j, 1], v.sk))), o.poly_mul(factor, new_key))
        assert (o.ntt_inv(got, _all(v)) == sr.lift(e, primes)).all(), (key_id, j)
    return retried


def check_relin_and_galois_keys(v, elts):
    lw, shape = v.hevm.lw, (v.D, 2, v.K, v.N)
    retried = check_kswitch_key(v, v.ll.read_device(lw.hevm_relin_key(v.hevm.vm), shape), sr.KEY_RELIN, v.o.poly_mul(v.sk, v.sk))
    for elt in elts:
        p = lw.hevm_galois_key(v.hevm.vm, elt)
        assert p, f"Galois key {elt} missing"
        retried += check_kswitch_key(v, v.ll.read_device(p, shape), sr.galois_key_id(elt), v.o.galois_ntt(v.sk, elt))
    return retried


def test_key_generation_60_bit(vm60):
    v = vm60
    assert sr.default_galois_elts(13) == list(dict.fromkeys(v.o.default_galois_elts()))   # (SEAL's list names the element N + 1 twice)
    retried = check_secret_and_public_key(v, sr.small_poly(v.keys["secret"], 0, v.N, sr.RNG_SK, kind="ternary"))
    retried += check_relin_and_galois_keys(v, sr.default_galois_elts(13))
    assert retried == 0          # a 60-bit draw is >= q with probability ~2^-35: the reference predicts no retry on this chain


def test_key_generation_narrow_primes_runs_the_retry_branch(vm46):
    """Retried coefficients the reference predicts (and the device must reproduce) for seed 0x4845564D on this chain: 8 in the
    relinearisation and Galois keys (23 keys x 4 digits x 5 limbs x 4096 coefficients, each retried with probability ~2^-18: 7.2 expected)."""
    v = vm46
    assert v.o.primes == NARROW and all(q.bit_length() == 46 and (1 << 46) - q < 1 << 28 for q in NARROW)
    check_secret_and_public_key(v, sr.small_poly(v.keys["secret"], 0, v.N, sr.RNG_SK, kind="ternary"))
    retried = check_relin_and_galois_keys(v, sr.default_galois_elts(12))
    print("retried coefficients compared:", retried)
    assert retried == RETRIED_46 and retried >= 4


def test_key_generation_grouped_digits(vm_grouped):
    """ks_special = 2, ks_alpha = 2 on 7 primes: 3 digits over the groups {0, 1}, {2, 3}, {4}; the key term sits on the group's limbs"""
    v = vm_grouped
    assert (v.D, v.L) == (3, 5)
    check_secret_and_public_key(v, sr.small_poly(v.keys["secret"], 0, v.N, sr.RNG_SK, kind="ternary"))
    check_relin_and_galois_keys(v, [sr.default_galois_elts(12)[3]])


def test_sparse_secrets_and_switching_keys(vm_sparse):
    v = vm_sparse
    K, N = v.K, v.N
    secret = sr.sparse_secret(v.keys["secret"], N, 32, sr.RNG_SK)
    assert int((secret != 0).sum()) == 32
    check_secret_and_public_key(v, secret)                                   # positions and signs
    down, up, limbs = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()   # (read as tests/test_gpu_sse.py reads them)
    assert v.hevm.lw.hevm_boot_switch_keys(v.hevm.vm, ctypes.byref(down), ctypes.byref(up), ctypes.byref(limbs)) == 1
    assert limbs.value == 2
    kd = v.ll.read_device(down.value, (1, 2, 2, N))                          # s -> s' over q0 and the special prime: one digit, two limbs
    ku = v.ll.read_device(up.value, (v.D, 2, K, N))                          # s' -> s over the chain
    a, _ = sr.uniform_poly(v.keys["pub"], sr.KEY_SWK_DOWN * 64 + 0, [v.o.primes[0], v.o.primes[K - 1]], N, sr.RNG_KSK_A)
    assert (kd[0, 1] == a).all()
    # swk_up in full: its new key is the ephemeral secret s', which the reference predicts too (RNG_ESK)
    esk = v.o.ntt_fwd(sr.lift(sr.sparse_secret(v.keys["secret"], N, 32, sr.RNG_ESK), v.o.primes), _all(v))
    check_kswitch_key(v, ku, sr.KEY_SWK_UP, esk)


def test_more_than_64_primes_are_refused_with_a_message():
    """the object numbering gives the limb and the digit 6 bits each (tests/test_sampler_reference.py): a context beyond that aborts
    with a message before anything is allocated (a child process: the library aborts)"""
    code = ("from dacapo_amd import lowlevel as ll\n"
            "ll.Context(12, 65)\n"
            "print('created')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "created" not in r.stdout, (r.returncode, r.stdout)
    assert "65 primes" in r.stderr and "at most 64 limbs and 64 digits per key" in r.stderr, r.stderr


# ---- encryption ----------------------------------------------------------------------------------------------------------------------------
def zero_encryption(v, obj, epoch, ell):
    """Encryptor's encryption of zero at `ell` primes from the reference's (u, e0, e1) at (obj, epoch) and the device's own pk:
    pk u + e over ell + 1 primes, divided and rounded by prime ell.  uint64[2][ell][N]"""
    o, cnt = v.o, ell + 1
    u, e0, e1 = (o.ntt_fwd(sr.lift(p, o.primes[:cnt]), list(range(cnt))) for p in sr.enc_sample(v.keys, obj, epoch, v.N))
    return np.stack([o.rescale_poly(o.poly_add(o.poly_mul(np.ascontiguousarray(v.pk[p, :cnt]), u), e)) for p, e in ((0, e0), (1, e1))])


def test_encrypt_equals_the_reference(vm60):
    from dacapo_amd import hevm_asm as ha

    v = vm60
    hevm, o, lw = v.hevm, v.o, v.hevm.lw
    levels = [2, v.L - 1, v.L]                                               # ell + 1 below, equal to the data primes, and the whole chain
    hv = ha.pack_hevm([40] * 3, levels, [40], [2], [3], 4, 0, v.L, np.array([(ha.OP_NEGATE, 3, 0, 0)], dtype=np.uint16))
    hevm.load_mem(ha.pack_cst([]), hv)
    x = [np.random.default_rng(20 + i).uniform(-1, 1, o.slots) for i in range(3)]
    lw.hevm_test_zero_encryption(hevm.vm, True)
    plain = []
    for i in range(3):
        hevm.setInput(i, x[i])                                               # the hook: (plaintext, 0), and no object is consumed
        ct = _get_ct(hevm, v.ll, i)
        assert ct.ell == levels[i] and not ct.data[1].any()
        plain.append(ct.data[0].copy())
    lw.hevm_test_zero_encryption(hevm.vm, False)

    def encrypt_and_check(i):
        hevm.setInput(i, x[i])
        got = _get_ct(hevm, v.ll, i)
        want = zero_encryption(v, v.encryptions, v.runs, levels[i])
        want[0] = o.poly_add(want[0], plain[i])
        v.encryptions += 1
        assert got.ell == levels[i] and got.scale == 2.0**40
        assert (got.data == want).all(), (i, v.encryptions - 1, v.runs)

    for i in (0, 1, 2, 0):                                                   # objects 0, 1, 2, 3 at epoch 0: the second encryption of input 0 differs
        encrypt_and_check(i)
    hevm.run()
    v.runs += 1
    for i in (1, 2):                                                         # objects 4, 5 at epoch 1
        encrypt_and_check(i)


# ---- opcode 10 ------------------------------------------------------------------------------------------------------------------------------
FORMS = {"captured graph": {}, "one lane, no graph": {"plan_lanes": 1, "plan_graph": 0}, "built graph": {"plan_graph": 2}, "loop": {"plan": 0}}


@pytest.mark.parametrize("form", list(FORMS))
def test_opcode10_zero_encryptions_are_fresh_in_every_run(form, tmp_path):
    from dacapo_amd import hevm_asm as ha

    v = _setup(SEED + 3, 13, num_primes=7, vm_options=FORMS[form])
    hevm, o, lw, ll = v.hevm, v.o, v.hevm.lw, v.ll
    E, MULCC, MULCP, RS, BOOT = ha.OP_ENCODE, ha.OP_MULCC, ha.OP_MULCP, ha.OP_RESCALE, ha.OP_BOOTSTRAP
    ops = [(E, 0, 0xFFFF, (2 << 10) + 20), (MULCC, 1, 0, 0), (MULCP, 2, 1, 0), (RS, 3, 2, 0),   # (the program of tests/test_gpu_opcode10.py)
           (BOOT, 4, 3, 3),                                                  # 1 prime -> 3 primes
           (BOOT, 5, 1, 5),                                                  # 2 primes -> 5 primes
           (BOOT, 6, 1, 3)]                                                  # 2 primes -> 3 primes: a plan encrypts it in one batch with the first
    outs = [(4, 3), (5, 5), (6, 3)]                                          # (register, target level) of the opcode-10 results
    hv = ha.pack_hevm([40], [2], [40, 40, 80, 80, 80], [1, 3, 2, 5, 3], [3, 4, 1, 5, 6], 7, 1, 2, np.array(ops, dtype=np.uint16))
    hevm.load_mem(ha.pack_cst([]), hv)
    hevm.setInput(0, np.random.default_rng(5).uniform(-1, 1, o.slots))       # a real ciphertext: Encryptor object 0
    v.encryptions += 1
    hevm.saveCtxt(0, tmp_path / "x.ct")

    def run():
        hevm.loadCtxt(0, tmp_path / "x.ct")                                 # the same input limbs in every run, whatever a run does to its registers
        hevm.run()
        v.runs += 1
        return [_get_ct(hevm, ll, r) for r, _ in outs]

    lw.hevm_test_zero_encryption(hevm.vm, True)
    first = run()                                                            # run 1: (pt', 0) -- and the epoch advances all the same
    for ct, (_, t) in zip(first, outs):
        assert ct.ell == t and not ct.data[1].any()
    lw.hevm_test_zero_encryption(hevm.vm, False)                             # (drops a recorded graph: run 2 records one with the zero-encryptions, run 3 replays it)
    diffs, cache = [], {}

    def zenc(obj, epoch, t):
        if (obj, epoch, t) not in cache:
            cache[(obj, epoch, t)] = zero_encryption(v, obj, epoch, t)
        return cache[(obj, epoch, t)]

    for n in (2, 3):
        epoch = v.runs
        assert epoch == n - 1
        got = run()
        diff = [np.stack([o.poly_sub(g.data[p], f.data[p]) for p in range(2)]) for g, f in zip(got, first)]
        if form == "loop":   # the one-instruction loop encrypts through Encryptor::encrypt: the objects that follow the input's, in program order
            objects = [[v.encryptions + k] for k in range(len(outs))]
            v.encryptions += len(outs)
        else:                # a plan numbers its opcode-10 items 2^32 + k in an order of its own
            objects = [[sr.PLAN_OBJECT0 + k for k in range(len(outs))]] * len(outs)
        used = []
        for d, (_, t), cand in zip(diff, outs, objects):
            match = [obj for obj in cand if (zenc(obj, epoch, t) == d).all()]
            assert len(match) == 1, (form, n, t, match)
            used += match
        assert sorted(used) == sorted({obj for cand in objects for obj in cand})   # every object exactly once
        diffs.append(diff)
    for d2, d3 in zip(*diffs):                                               # out_3 - out_2 != 0: the replayed run drew fresh randomness
        assert (d2 != d3).any() and (d2[0] != d3[0]).mean() > 0.99
    hevm.close()
