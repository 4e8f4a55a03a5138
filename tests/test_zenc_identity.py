"""The identity behind option zenc_head = 1 (dacapo_amd/csrc/hevm_vm.hip HEVM::plan_zero_encrypt), on the oracle's own functions, no GPU:
an encryption of zero at l primes is rescale(pk * NTT(u) + NTT(e)) over l + 1 primes, D = l the dropped one -- 5l + 5 transforms.  The same
canonical residues come out of 3l + 3, because the transforms are linear and every step is exact mod q_i:
    U_i     = NTT_i([u]_{q_i})                                       i = 0..l
    delta_p = iNTT_D(pk_{p,D} * U_D) + [e_p]_{q_D}                   (e_p is never transformed at D)
    rho_p   = [delta_p + floor(q_D/2)]_{q_D},   t_{p,i} = (rho_p mod q_i) - (floor(q_D/2) mod q_i)
    z_{p,i} = q_D^-1 (pk_{p,i} * U_i - NTT_i(t_{p,i} - [e_p]_{q_i}))     i < l    (one lifted polynomial per kept limb carries the noise)
Checked with == against Oracle.rescale_poly at N = 2^10 for l = 1, 3 and L (the dropped prime is then the special prime), with random
u in {-1, 0, 1} and e in [-21, 21], with e = +-21 everywhere, and with pk crafted so that delta + floor(q_D/2) lands on 0, q_D - 1,
floor(q_D/2) and floor(q_D/2) +- 1 -- the wrap and the sign change of the rounding."""
import numpy as np
import pytest

import sampler_reference as sr
from oracle.oracle import Oracle

LOGN, K = 10, 5


@pytest.fixture(scope="module")
def o():
    return Oracle(LOGN, K)


def reference(o, pk, u, e, l):
    """rescale_poly(pk * NTT(u) + NTT(e)) over primes 0..l: uint64[l][N]"""
    cnt = l + 1
    idx, q = list(range(cnt)), o.primes[:cnt]
    return o.rescale_poly(o.poly_add(o.poly_mul(pk, o.ntt_fwd(sr.lift(u, q), idx)), o.ntt_fwd(sr.lift(e, q), idx)))


def identity(o, pk, u, e, l):
    """the four lines above; also returns rho (for the tests that aim at its edge values)"""
    cnt, D, N = l + 1, l, o.N
    q = o.primes[:cnt]
    qD, half = q[D], q[D] >> 1
    prod = o.poly_mul(pk, o.ntt_fwd(sr.lift(u, q), list(range(cnt))))             # pk_i * U_i, every limb
    delta = (o.ntt_inv(prod[D:D + 1], [D])[0] + sr.lift(e, [qD])[0]) % np.uint64(qD)
    rho = (delta + np.uint64(half)) % np.uint64(qD)
    w = np.empty((l, N), dtype=np.uint64)
    inv = np.empty((l, N), dtype=np.uint64)
    for i in range(l):
        qi = np.uint64(q[i])
        t = (rho % qi + qi - np.uint64(half % q[i])) % qi
        w[i] = (t + qi - sr.lift(e, [q[i]])[0]) % qi                              # t_i - [e]_{q_i}
        inv[i] = pow(qD, -1, q[i])
    return o.poly_mul(o.poly_sub(prod[:l], o.ntt_fwd(w, list(range(l)))), inv), rho


def random_pk(o, rng, cnt):
    return np.stack([rng.integers(0, o.primes[i], o.N, dtype=np.uint64) for i in range(cnt)])


@pytest.mark.parametrize("l", [1, 3, K - 1])
def test_identity_on_random_draws(o, l):
    rng = np.random.default_rng(100 + l)
    for _ in range(2):                                                            # the two polynomials of a ciphertext: two keys, two noises
        pk, u, e = random_pk(o, rng, l + 1), rng.integers(-1, 2, o.N), rng.integers(-21, 22, o.N)
        assert (identity(o, pk, u, e, l)[0] == reference(o, pk, u, e, l)).all()


@pytest.mark.parametrize("l", [1, 3, K - 1])
@pytest.mark.parametrize("sign", [1, -1])
def test_identity_with_the_largest_noise_everywhere(o, l, sign):
    rng = np.random.default_rng(200 + l)
    pk, u, e = random_pk(o, rng, l + 1), rng.integers(-1, 2, o.N), np.full(o.N, 21 * sign)
    assert (identity(o, pk, u, e, l)[0] == reference(o, pk, u, e, l)).all()


@pytest.mark.parametrize("l", [1, 3, K - 1])
def test_identity_at_the_wrap_and_the_sign_change_of_the_rounding(o, l):
    """pk's limb at the dropped prime is solved for: pk_D = NTT_D(delta* - e) / U_D pointwise, with delta* + floor(q_D/2) set to the edge
    values in the first coefficients (random elsewhere)"""
    rng = np.random.default_rng(300 + l)
    D, N = l, o.N
    qD, half = o.primes[D], o.primes[D] >> 1
    u, e = rng.integers(-1, 2, N), rng.integers(-21, 22, N)
    UD = o.ntt_fwd(sr.lift(u, [qD]), [D])[0]
    assert UD.all()                                                               # invertible pointwise
    edges = [0, qD - 1, half, half + 1, half - 1]
    rho_want = rng.integers(0, qD, N, dtype=np.uint64)
    rho_want[: 2 * len(edges)] = edges + edges                                    # each edge under two different noise values
    c = (rho_want + np.uint64(qD - half) + np.uint64(qD) - sr.lift(e, [qD])[0]) % np.uint64(qD)   # delta* - e
    chat = o.ntt_fwd(c[None], [D])[0]
    pk = random_pk(o, rng, l + 1)
    pk[D] = [int(a) * pow(int(b), -1, qD) % qD for a, b in zip(chat, UD)]
    got, rho = identity(o, pk, u, e, l)
    assert (rho == rho_want).all()                                                # the crafted key does land on the edges
    assert (got == reference(o, pk, u, e, l)).all()
