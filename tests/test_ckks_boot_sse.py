"""CPU: sparse-secret encapsulation in the bootstrapping lowering (ckks_boot.py sse=True, opcode 20 = hevm_asm.OP_KEYSWITCH).
ModRaise is wrapped in KEYSWITCH 0 (main secret -> ephemeral sparse secret, at 1 prime) and KEYSWITCH 1 (back, at the top level); nothing
else of the program changes."""
import gzip
from pathlib import Path

import numpy as np

from dacapo_amd import ckks_boot as cb
from dacapo_amd import hevm_asm as ha

GOLDEN = Path(__file__).resolve().parent / "golden"


def _one_bootstrap(logN, sse):
    _, cst, hv, offs, em = cb.single_bootstrap_program(logN, sse=sse)
    return cst, hv, offs, em


def test_sse_adds_exactly_two_keyswitches_around_modraise():
    cst0, hv0, offs0, _ = _one_bootstrap(11, False)
    cst1, hv1, offs1, em = _one_bootstrap(11, True)
    o0, o1 = ha.unpack_hevm(hv0)["ops"], ha.unpack_hevm(hv1)["ops"]
    assert len(o1) == len(o0) + 2
    ks = np.nonzero(o1[:, 0] == ha.OP_KEYSWITCH)[0]
    mr = np.nonzero(o1[:, 0] == ha.OP_MODRAISE)[0]
    assert len(ks) == 2 and len(mr) == 1
    down, up = o1[ks[0]], o1[ks[1]]
    assert ks[0] == mr[0] - 1 and ks[1] == mr[0] + 1                     # immediately before and after ModRaise
    assert int(down[3]) == 0 and int(up[3]) == 1                           # rhs: 0 = s -> s', 1 = s' -> s
    assert int(o1[mr[0], 2]) == int(down[1]) and int(up[2]) == int(o1[mr[0], 1])   # a chain: keyswitch -> modraise -> keyswitch
    assert offs1 == offs0 and cst1 == cst0
    assert int((o0[:, 0] == ha.OP_KEYSWITCH).sum()) == 0                   # off by default


def test_sse_program_simulates_like_the_plain_one():
    logN = 11
    K = 3 + cb.boot_levels() + 1
    primes = cb.seal_prime_chain(logN, K)
    cst0, hv0, _, _ = _one_bootstrap(logN, False)
    cst1, hv1, _, _ = _one_bootstrap(logN, True)
    msg = np.random.default_rng(4).uniform(-1, 1, 1 << (logN - 1))
    # the same overflow distribution on both sides: the SSE program's ModRaise runs under the ephemeral weight
    out0 = cb.simulate(hv0, cst0, [msg], logN, primes, secret_weight=32)[0]
    out1 = cb.simulate(hv1, cst1, [msg], logN, primes, secret_weight=192, boot_secret_weight=32)[0]
    assert np.abs(out1 - out0).max() < 1e-8
    assert np.abs(out1.real - msg).max() < 1e-3
    _, tr = cb.simulate(hv1, cst1, [msg], logN, primes, boot_secret_weight=32, return_trace=True)
    ks_levels = [l for opc, _, l, _ in tr if opc == ha.OP_KEYSWITCH]
    assert ks_levels == [1, K - 1]                                          # level unchanged by the switch itself


def test_lowering_the_b14_fixture_with_sse_keeps_the_rotation_set():
    fx = ha.read_fixture(GOLDEN / "resnet20_nt16")
    hv = gzip.open(GOLDEN / "resnet20_nt16.b14.hevm.gz").read()
    logN = 17
    targets = {int(r) for o, _, _, r in ha.unpack_hevm(hv)["ops"].tolist() if o == ha.OP_BOOTSTRAP}
    assert len(targets) == 1
    ks = 9
    KB = targets.pop() + cb.boot_levels() + ks
    hv0, cst0 = cb.lower_bootstraps(hv, fx["cst"], logN, KB, msg_bits=4, ks=ks)
    hv1, cst1 = cb.lower_bootstraps(hv, fx["cst"], logN, KB, msg_bits=4, ks=ks, sse=True)
    o0, o1 = ha.unpack_hevm(hv0)["ops"], ha.unpack_hevm(hv1)["ops"]
    n_boot = int((o0[:, 0] == ha.OP_MODRAISE).sum())
    assert n_boot == 38
    assert int((o1[:, 0] == ha.OP_KEYSWITCH).sum()) == 2 * n_boot and len(o1) == len(o0) + 2 * n_boot
    assert cb.rotation_offsets(hv1) == cb.rotation_offsets(hv0)
    assert cst1 == cst0


def test_scale_mirror_passes_keyswitch_through():
    logN = 11
    K = 3 + cb.boot_levels() + 1
    b = ha.Builder(slots=1 << (logN - 1), init_level=1, shadow=False)
    x = b.input(None, level=1, scale_bits=40)
    em = cb.BootstrapEmitter(b, logN, K, 3, sse=True)
    y, label = em.bootstrap(x, 2.0**40)
    sc = cb.vm_scales(b, em.primes)
    assert sc[y.id] == label == 2.0**40
    for op in b.ops:
        if op.opcode == ha.OP_KEYSWITCH:
            assert sc[op.dst] == sc[op.lhs]
