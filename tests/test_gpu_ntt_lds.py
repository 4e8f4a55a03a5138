"""GPU parity of the single-launch LDS-resident NTT for N = 2^12 .. 2^14 (csrc/ntt_lds.hip, reached through dc_ntt_variant(variant = 1) and,
from the limb counts of options ntt_lds_min_limbs / ntt_lds_inv_min_limbs on, through dc_ntt_forward / dc_ntt_inverse): every output ==
the CPU oracle and == the two-launch tiles, bit for bit."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.oracle import Oracle, splitmix_fill

RINGS = [12, 13, 14]


@functools.lru_cache(maxsize=None)
def _ring(logN, K=3):
    from dacapo_amd import lowlevel as ll

    return ll, ll.Context(logN, K), Oracle(logN, K)


def _lds_ring(logN):
    ll, ctx, o = _ring(logN)
    assert ctx.ntt_variant_supported(1)  # (asked first: dc_ntt_variant aborts the process on a ring it does not serve)
    return ll, ctx, o


def _both_ways(ll, ctx, o, a, pidx, **how):
    """forward and inverse of the limbs `a` through variant 1 == oracle, and each round trip is exact"""
    for inverse, want in ((False, o.ntt_fwd(a, pidx)), (True, o.ntt_inv(a, pidx))):
        d = ll.DeviceBuffer.from_host(a)
        ctx.ntt(d, len(pidx), inverse=inverse, variant=1, **how)
        assert (d.to_host() == want).all(), ("inverse" if inverse else "forward")
        ctx.ntt(d, len(pidx), inverse=not inverse, variant=1, **how)
        assert (d.to_host() == a).all(), ("round trip from the " + ("inverse" if inverse else "forward"))


@pytest.mark.parametrize("logN,yes", [(12, True), (13, True), (14, True), (15, True), (16, False)])
def test_support_query(logN, yes):
    _, ctx, _ = _ring(logN)
    assert ctx.ntt_variant_supported(0) and ctx.ntt_variant_supported(1) == yes


@pytest.mark.parametrize("logN", RINGS)
def test_matches_oracle_on_an_irregular_prime_pattern(logN):
    ll, ctx, o = _lds_ring(logN)
    N, pidx = 1 << logN, [0, 1, 2, 2, 0]  # through the device index array
    a = np.stack([splitmix_fill(0x1D5 + b, N) % np.uint64(o.primes[p]) for b, p in enumerate(pidx)])
    a[0, : N // 2] = 0
    a[1, :] = np.uint64(o.primes[pidx[1]] - 1)
    _both_ways(ll, ctx, o, a, pidx, prime_idx=ll.DeviceBuffer.from_host(np.array(pidx, dtype=np.int32)))


@pytest.mark.parametrize("logN", RINGS)
@pytest.mark.parametrize("inverse", [False, True])
def test_limb_stride_and_arithmetic_prime_pattern(logN, inverse):
    ll, ctx, o = _lds_ring(logN)
    N, pidx = 1 << logN, [1 + b % 2 for b in range(5)]
    s = np.full((5, 2, N), 0xDEADBEEF, dtype=np.uint64)  # stride 2N: the second halves are not limbs
    for b, p in enumerate(pidx):
        s[b, 0] = splitmix_fill(b + 11, N) % np.uint64(o.primes[p])
    d = ll.DeviceBuffer.from_host(s)
    ctx.ntt(d, 5, inverse=inverse, prime_base=1, prime_period=2, limb_stride=2 * N, variant=1)
    got = d.to_host()
    assert (got[:, 1] == np.uint64(0xDEADBEEF)).all()
    assert (got[:, 0] == (o.ntt_inv if inverse else o.ntt_fwd)(s[:, 0], pidx)).all()


@pytest.mark.parametrize("logN,limbs", [(12, 1291), (13, 1037), (14, 521)])
def test_more_limbs_than_resident_workgroups(logN, limbs):
    """256 CUs hold 1280 / 512 / 256 workgroups of the three rings: each count exceeds that and is no multiple of it, so the persistent
    grid's workgroups walk over one, two or three limbs each"""
    ll, ctx, o = _lds_ring(logN)
    K, N = 3, 1 << logN
    q = np.array([o.primes[b % K] for b in range(limbs)], dtype=np.uint64)[:, None]
    big = np.random.default_rng(logN).integers(0, 1 << 62, size=(limbs, N), dtype=np.uint64) % q
    check = [0, 1, 2, 255, 256, limbs // 2, limbs - 2, limbs - 1]
    for inverse in (False, True):
        outs = []
        for variant in (0, 1):
            d = ll.DeviceBuffer.from_host(big)
            ctx.ntt(d, limbs, inverse=inverse, prime_base=0, prime_period=K, variant=variant)
            outs.append(d.to_host())
        assert (outs[0] == outs[1]).all()
        assert (outs[1][check] == (o.ntt_inv if inverse else o.ntt_fwd)(big[check], [b % K for b in check])).all()


@pytest.mark.parametrize("logN", RINGS)
def test_default_entry_takes_it_from_the_option_on(logN, request):
    from dacapo_amd import runner

    ll, ctx, o = _ring(logN)
    names = ("ntt_lds_min_limbs", "ntt_lds_inv_min_limbs")
    for name, old in [(n, runner.get_option(n)) for n in names]:
        request.addfinalizer(lambda name=name, old=old: runner.set_option(name, old))
    N = 1 << logN
    a = np.stack([splitmix_fill(77 + b, N) % np.uint64(o.primes[b]) for b in range(3)])
    outs = []
    for threshold in (0, 1):
        for name in names:
            runner.set_option(name, threshold)
        d = ll.DeviceBuffer.from_host(a)
        ctx.ntt(d, 3)
        outs.append(d.to_host())
        ctx.ntt(d, 3, inverse=True)
        assert (d.to_host() == a).all()
    assert (outs[0] == outs[1]).all() and (outs[1] == o.ntt_fwd(a, [0, 1, 2])).all()


def test_generic_width_build_on_a_mixed_chain():
    from dacapo_amd import lowlevel as ll
    from test_gpu_prime_widths import _chain

    logN, N = 13, 1 << 13
    primes = _chain(logN, [60, 51, 51, 60])
    ctx, o = ll.Context(logN, primes=primes), Oracle(logN, len(primes), primes=primes)
    assert ctx.L is ll.lib_gw() and ctx.ntt_variant_supported(1)
    a = np.stack([splitmix_fill(17 + i, N) % np.uint64(p) for i, p in enumerate(primes)])
    a[1, :] = np.uint64(primes[1] - 1)
    _both_ways(ll, ctx, o, a, list(range(len(primes))))
