"""GPU: the base conversions of grouped-digit key switching on the matrix cores for digits and special sets of 9..16 primes
(dacapo_amd/csrc/hybrid_ks.hip hyb_conv_mfma_wide_kernel: two K-chunks of 64 bytes per dot product).  A rotation hop and a ct x ct multiply +
relinearise on the oracle's keys == the oracle's limbs, with the conversions on the matrix cores and (option hyb_mfma = 0) on the vector
units, and dc_context_conv_matrix_cores says which of the two a level takes."""
import numpy as np
import pytest

from gpu_helpers import _get_ct, _import_keys, _mirror_vm
from oracle.oracle import Ciphertext, Oracle, splitmix_fill

pytestmark = pytest.mark.gpu
LOGN, N = 12, 1 << 12
# (28, 12, 9): one input in the mod-up's second chunk, the mod-down on the 32-deep tail; (30, 13, 11): the mod-down just past that tail;
# (36, 16, 16): both chunks full, 20 data primes = a full digit and a partial one of 4
SHAPES = [(28, 12, 9), (30, 13, 11), (36, 16, 16)]
_RINGS: dict = {}


def _ring(K, ks, alpha, primes=None):
    """oracle with its keys, and its results per (level, operand form): made once, left unchanged"""
    key = (K, ks, alpha, primes is None)
    if key not in _RINGS:
        o = Oracle(LOGN, K, primes=primes)
        o.set_hybrid(ks, alpha)
        o.keygen(seed=0x4845564D, galois_elts=[o.elt_from_step(5)])
        _RINGS[key] = (o, {})
    return _RINGS[key]


def _case(o, cache, ell, form):
    """operands (random residues | q - 1 in every limb) and the oracle's rotation and product of them"""
    if (ell, form) not in cache:
        q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
        a, b = (np.stack([np.stack([splitmix_fill(s + 7 * p + i + 100 * ell, N) for i in range(ell)]) % q for p in range(2)]) for s in (1, 99))
        if form == "edge":
            a[:], b[:] = q - np.uint64(1), q - np.uint64(1)
        A, B = Ciphertext(a, 2.0**40), Ciphertext(b, 2.0**40)
        cache[ell, form] = (a, b, o.apply_galois(A, o.elt_from_step(5)).data, o.mul_relin(A, B).data)
    return cache[ell, form]


def _check(K, ks, alpha, fuse, primes=None):
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    o, cache = _ring(K, ks, alpha, primes)
    elt, top = o.elt_from_step(5), K - ks
    # first matrix-core level (chunk 1 all zero); first live input of chunk 1; a full digit; + a one-input digit; several output blocks
    levels = sorted({4, 9, alpha, alpha + 1, top})
    for mfma in (1, 0):
        with runner.options(hyb_fuse=fuse, hyb_mfma=mfma):
            ctx = ll.Context(LOGN, K, primes=primes, special=ks, alpha=alpha)
            assert ctx.primes == o.primes and ctx.key_digits == o.dnum
            L = ctx.L
            assert [L.dc_context_conv_matrix_cores(ctx.h, ell) for ell in [3] + levels] == [0] + [mfma] * len(levels)
            dk, dr = ll.DeviceBuffer.from_host(o.galois[elt]), ll.DeviceBuffer.from_host(o.relin)
            for ell in levels:
                for form in ("random", "edge"):
                    a, b, rot, mul = _case(o, cache, ell, form)
                    da, db, dd = ll.DeviceBuffer.from_host(a), ll.DeviceBuffer.from_host(b), ll.DeviceBuffer((2, ell, N))
                    L.dc_ct_rotate_hop(ctx.h, dd.ptr, ell * N, da.ptr, ell * N, elt, dk.ptr, ell, None)
                    assert (dd.to_host() == rot).all(), ("rotate", mfma, ell, form)
                    L.dc_ct_mul_relin(ctx.h, dd.ptr, ell * N, da.ptr, ell * N, db.ptr, ell * N, dr.ptr, ell, None)
                    assert (dd.to_host() == mul).all(), ("mul_relin", mfma, ell, form)
    return L


# hyb_fuse 2 / 0: the conversions on pre-scaled / plain inputs; 1 (once, at 16 inputs): the conversions in the transforms' loaders
@pytest.mark.parametrize("shape,fuse", [(s, f) for s in SHAPES for f in (2, 0)] + [(SHAPES[2], 1)])
def test_wide_digit_conversions_match_the_oracle_on_either_unit(shape, fuse):
    _check(*shape, fuse)


def test_mixed_width_chain_on_the_generic_width_build():
    from test_gpu_prime_widths import _chain

    from dacapo_amd import lowlevel as ll

    assert _check(30, 13, 11, 2, _chain(LOGN, [60] + [51] * 16 + [60] * 13)) is ll.lib_gw()


def test_vm_program_under_16_special_primes_matches_the_oracle_vm(tmp_path):
    from test_gpu_hybrid import _program

    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    K, ks = 36, 16
    hevm = runner.HEVM(seed=77, logN=LOGN, num_primes=K, ks_special=ks, ks_alpha=ks, vm_options={"plan": 1, "plan_graph": 1})
    assert hevm.max_level == K - ks and hevm.key_digits == 2
    assert ll.lib().dc_context_conv_matrix_cores(hevm.ctx_handle, K - ks) == 1
    o = Oracle(LOGN, K)
    o.set_hybrid(ks, ks)
    _import_keys(o, hevm, ll)
    b = _program(1 << (LOGN - 1), K - ks, 5)
    cst, hv, _ = b.assemble()
    hevm.load_mem(cst, hv)
    ovm = _mirror_vm(hevm, ll, o, cst, hv, tmp_path)
    for i, a in enumerate(b.args):
        hevm.setInput(i, a.plain)
        ovm.ciphers[i] = _get_ct(hevm, ll, i)
    hevm.run()
    ovm.run()
    r = ovm.prog.res_dst[0]
    got, want = _get_ct(hevm, ll, r), ovm.ciphers[r]
    assert got.ell == want.ell and got.scale == want.scale and (got.data == want.data).all()
    hevm.close()
