"""GPU: the zero-encryptions a plan makes at the start of run() (dacapo_amd/csrc/hevm_vm.hip HEVM::plan_zero_encrypt) with option
zenc_head = 1 -- only u is transformed; the public key's product and the noise ride on the divide-and-round (tests/test_zenc_identity.py
restates the identity on the CPU) -- and with zenc_head = 0, Encryptor::encrypt's sequence batched, against the host reference of the
samplers (tests/sampler_reference.py) on the hooks build.  The method is tests/test_gpu_samplers.py's: a run with the
hevm_test_zero_encryption hook on gives the plaintext half of every opcode-10 result; a normal run's result minus that must equal the
predicted zero-encryption of exactly one candidate object at the run's epoch, every candidate used exactly once.  Every comparison is ==.
  * N = 2^12, 7 primes, both values of the option, as a captured graph and on one lane without a graph: seven items -- five to 3 primes, one
    to 1 prime, one to the top level (the dropped prime is the special prime) -- with the head's chunk forced to 2 items (the hooks build's
    HEVM_TEST_ZENC_CHUNK), so the five split 2 + 2 + 1; two consecutive runs (the epoch advances; a graph replay);
  * N = 2^15, 14 primes, ntt_full_min_limbs = 4: the 8 limbs of u of a two-item chunk go through the single-crossing transform;
  * N = 2^12, two streams: three items to 3 primes per stream, the six results match six distinct objects."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sampler_reference as sr  # noqa: E402
from gpu_helpers import _get_ct  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

SEED = 0x4845564D


def _setup(logN, num_primes, vm_options, chunk):
    from types import SimpleNamespace

    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    os.environ["HEVM_TEST_ZENC_CHUNK"] = str(chunk)       # read by hevm_init_seeded (csrc/test_hooks.hip)
    try:
        hevm = runner.HEVM(seed=SEED + 7, logN=logN, num_primes=num_primes, vm_options=vm_options)
    finally:
        del os.environ["HEVM_TEST_ZENC_CHUNK"]
    o = Oracle(logN, hevm.K)
    v = SimpleNamespace(hevm=hevm, ll=ll, o=o, K=hevm.K, N=hevm.N, L=hevm.max_level, keys=sr.rng_keys_from_test_seed(SEED + 7))
    v.pk = ll.read_device(hevm.lw.hevm_public_key(hevm.vm), (2, hevm.K, hevm.N))
    return v


def zero_encryption(v, obj, epoch, ell):
    """Encryptor's encryption of zero at `ell` primes from the reference's (u, e0, e1) at (obj, epoch) and the device's own pk:
    pk u + e over ell + 1 primes, divided and rounded by prime ell.  uint64[2][ell][N]  (tests/test_gpu_samplers.py, restated)"""
    o, cnt = v.o, ell + 1
    u, e0, e1 = (o.ntt_fwd(sr.lift(p, o.primes[:cnt]), list(range(cnt))) for p in sr.enc_sample(v.keys, obj, epoch, v.N))
    return np.stack([o.rescale_poly(o.poly_add(o.poly_mul(np.ascontiguousarray(v.pk[p, :cnt]), u), e)) for p, e in ((0, e0), (1, e1))])


def _program(targets):
    """x * x at 2 primes, then one opcode 10 per entry of `targets` from it (registers 2, 3, ...)"""
    from dacapo_amd import hevm_asm as ha

    ops = [(ha.OP_ENCODE, 0, 0xFFFF, (2 << 10) + 20), (ha.OP_MULCC, 1, 0, 0)]
    ops += [(ha.OP_BOOTSTRAP, 2 + k, 1, t) for k, t in enumerate(targets)]
    n = len(targets)
    hv = ha.pack_hevm([20], [2], [40] * n, list(targets), [2 + k for k in range(n)], 2 + n, 1, 2, np.array(ops, dtype=np.uint16))
    return ha.pack_cst([]), hv


def _check_runs(v, targets, streams, runs, tmp_path):
    """the hook run, then `runs` normal runs: every result's zero-encryption half is one of the plan's objects at that run's epoch"""
    hevm, o, lw, ll = v.hevm, v.o, v.hevm.lw, v.ll
    if streams > 1:
        hevm.set_streams(streams)
    hevm.load_mem(*_program(targets))
    for q in range(streams):
        hevm.select_stream(q)
        hevm.setInput(0, np.random.default_rng(5 + q).uniform(-1, 1, o.slots))
        hevm.saveCtxt(0, tmp_path / f"x{q}.ct")
    outs = [(q, 2 + k, t) for q in range(streams) for k, t in enumerate(targets)]
    epoch = 0

    def run():
        for q in range(streams):                            # the same input limbs in every run
            hevm.select_stream(q)
            hevm.loadCtxt(0, tmp_path / f"x{q}.ct")
        hevm.run()
        got = []
        for q, r, _ in outs:
            hevm.select_stream(q)
            got.append(_get_ct(hevm, ll, r))
        return got

    lw.hevm_test_zero_encryption(hevm.vm, True)
    first = run()                                           # (plaintext, 0); the epoch advances all the same
    epoch += 1
    for ct, (_, _, t) in zip(first, outs):
        assert ct.ell == t and not ct.data[1].any()
    lw.hevm_test_zero_encryption(hevm.vm, False)
    cache, diffs = {}, []
    objects = [sr.PLAN_OBJECT0 + k for k in range(len(outs))]
    for n in range(runs):
        got = run()
        used = []
        diff = [np.stack([o.poly_sub(g.data[p], f.data[p]) for p in range(2)]) for g, f in zip(got, first)]
        for d, (q, r, t) in zip(diff, outs):
            for obj in objects:
                if (obj, t) not in cache:
                    cache[(obj, t)] = zero_encryption(v, obj, epoch, t)
            match = [obj for obj in objects if (cache[(obj, t)] == d).all()]
            assert len(match) == 1, (n, q, r, t, match)
            used += match
        assert sorted(used) == objects                      # every object exactly once
        diffs.append(diff)
        epoch += 1
        cache.clear()
    return diffs


FORMS = {"captured graph": {}, "one lane, no graph": {"plan_lanes": 1, "plan_graph": 0}}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("head", [1, 0])
def test_chunked_head_makes_the_predicted_zero_encryptions(head, form, tmp_path):
    v = _setup(12, 7, dict(FORMS[form], zenc_head=head), chunk=2)
    assert v.L == 6
    try:
        d2, d3 = _check_runs(v, [3, 3, 3, 3, 3, 1, v.L], 1, 2, tmp_path)
        for a, b in zip(d2, d3):                            # the second run (a graph replay) drew fresh randomness
            assert (a[0] != b[0]).mean() > 0.99
    finally:
        v.hevm.close()


def test_head_through_the_single_crossing_transform(tmp_path):
    from dacapo_amd import runner

    with runner.options(ntt_full_min_limbs=4):
        v = _setup(15, 14, {"zenc_head": 1}, chunk=2)
        try:
            _check_runs(v, [3, 3], 1, 1, tmp_path)
        finally:
            v.hevm.close()


def test_head_with_two_streams(tmp_path):
    v = _setup(12, 7, {"zenc_head": 1}, chunk=2)
    try:
        _check_runs(v, [3, 3, 3], 2, 1, tmp_path)
    finally:
        v.hevm.close()
