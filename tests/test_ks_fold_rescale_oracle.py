"""A rescale folded into the multiply's key switch (option ks_fold_rescale, dc_ct_mul_relin_rescale; dacapo_amd/csrc/fused_ks.hip
f_dr2_icols_lift_fcols_kernel), the part that needs no GPU: the one-pass division by P q_{l-1} restated on the oracle's building blocks and
Python integers equals rescale(mul_plain(add_plain(mul_relin(a, b), A), S)) limb for limb.

Notation (SEAL layout, one special prime P = q_{K-1}, level l, L = l - 1): X the key-switch inner products (NTT form), d the tensor term,
A a plaintext added to c0, s_i the residue of a CONSTANT polynomial that multiplies the result.
    rho = [iNTT_P(X_P) + floor(P/2)]_P                    t_i = (rho mod q_i) - (floor(P/2) mod q_i)
    c_L = s_L (iNTT_L(X_L + P (d_L + A_L)) - t_L) P^-1    u = [c_L + floor(q_L/2)]_{q_L},  u_i = (u mod q_i) - (floor(q_L/2) mod q_i)
    v_i = (s_i P^-1 t_i + u_i) q_L^-1                      r_i = s_i q_L^-1 (X_i P^-1 + d_i + A_i) - NTT_i(v_i)
The multiplier has to be constant so that it commutes with the transform; the all-ones upscale constant of the traced programs encodes to
exactly that, which is asserted here too."""
import numpy as np
import pytest

from oracle.oracle import Ciphertext, Oracle, splitmix_fill

_ORACLES: dict = {}


def _oracle(logN, K):
    if (logN, K) not in _ORACLES:
        o = Oracle(logN, K)
        o.keygen(seed=0x4845564D, galois_elts=[], relin=True)
        _ORACLES[(logN, K)] = o
    return _ORACLES[(logN, K)]


def _ct(o, ell, seed):
    q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
    return Ciphertext(np.stack([np.stack([splitmix_fill(seed + 7 * p + i, o.N) for i in range(ell)]) % q for p in range(2)]), 2.0**40)


def folded_mul_relin_rescale(o, a, b, A=None, s=None):
    """the identity of the module docstring -> [2][l - 1][N].  A: [l][N] limbs or None; s: l residues or None"""
    ell, K, N = a.ell, o.K, o.N
    L, q, P = ell - 1, [int(x) for x in o.primes], int(o.primes[K - 1])
    s = [1] * ell if s is None else [int(x) for x in s]
    t3 = o.tensor(a, b)
    X = o.keyswitch_inner_simple(t3[2], o.relin)  # [2][l + 1][N]: data primes, then the special prime
    out = np.zeros((2, L, N), dtype=np.uint64)
    for p in range(2):
        d = t3[p].astype(object)
        Ap = A.astype(object) if (A is not None and p == 0) else np.zeros((ell, N), dtype=object)
        rho = (o.ntt_inv(X[p, ell][None], [K - 1])[0].astype(object) + P // 2) % P
        t = lambda i: (rho % q[i] - (P // 2) % q[i]) % q[i]  # noqa: E731
        row = ((X[p, L].astype(object) + P * (d[L] + Ap[L])) % q[L]).astype(np.uint64)
        cL = s[L] * (o.ntt_inv(row[None], [L])[0].astype(object) - t(L)) * pow(P, -1, q[L]) % q[L]
        u = (cL + q[L] // 2) % q[L]
        for i in range(L):
            pinv, qinv = pow(P, -1, q[i]), pow(q[L], -1, q[i])
            ui = (u % q[i] - (q[L] // 2) % q[i]) % q[i]
            v = ((s[i] * pinv * t(i) + ui) * qinv % q[i]).astype(np.uint64)
            r = (s[i] * qinv * (X[p, i].astype(object) * pinv + d[i] + Ap[i]) - o.ntt_fwd(v[None], [i])[0].astype(object)) % q[i]
            out[p, i] = r.astype(np.uint64)
    return out


@pytest.mark.parametrize("logN,K,ell", [(10, 4, 2), (10, 4, 3), (11, 6, 5), (10, 14, 13)])
def test_one_pass_division_equals_the_two_roundings(logN, K, ell):
    o = _oracle(logN, K)
    a, b = _ct(o, ell, 1 + 100 * ell), _ct(o, ell, 99 + 100 * ell)
    prod = o.mul_relin(a, b)
    # without "+ plaintext" and "* constant"
    assert (folded_mul_relin_rescale(o, a, b) == o.rescale(prod).data).all()
    # with both: A random canonical limbs, S the oracle's encoding of the all-ones vector
    A = _ct(o, ell, 777).data[0]
    S = o.encode(np.ones(o.slots), 2.0**20, ell)
    assert (S.data == S.data[:, :1]).all()  # a constant polynomial: every NTT value of a limb is the same
    from oracle.oracle import Plaintext

    want = o.rescale(o.mul_plain(o.add_plain(prod, Plaintext(A, prod.scale)), S))
    assert (folded_mul_relin_rescale(o, a, b, A, S.data[:, 0]) == want.data).all()
    # and a square
    assert (folded_mul_relin_rescale(o, a, a) == o.rescale(o.mul_relin(a, a)).data).all()


@pytest.mark.parametrize("logN", [12, 15])
@pytest.mark.parametrize("bits", [20, 40, 60, 80])
def test_the_all_ones_constant_encodes_to_a_constant_polynomial(logN, bits):
    """what lets the plan decide from the limbs: the upscale constant of the traced programs (EncItem.len == 0) has equal values in a limb"""
    o = Oracle(logN, 4)
    S = o.encode(np.ones(o.slots), 2.0**bits, 3)
    assert (S.data == S.data[:, :1]).all()
    assert [int(x) for x in S.data[:, 0]] == [(1 << bits) % int(q) for q in o.primes[:3]]


def test_ks_fold_rescale_is_a_known_option_with_default_zero():
    import re
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    table = (root / "dacapo_amd" / "csrc" / "options.cpp").read_text()
    assert re.search(r'\{\s*"ks_fold_rescale",\s*0\s*\}', table)
    assert "OPT_KS_FOLD_RESCALE" in (root / "dacapo_amd" / "csrc" / "options.hpp").read_text()
