"""A rescale folded into the grouped-digit multiply's mod-down (option hyb_fold_rescale; dacapo_amd/csrc/hybrid_fused.hip
hybf_mul_relin_rescale_tail), the part that needs no GPU: the identity the kernels implement, restated on the oracle's primitives and Python
integers, equals rescale(mul_relin(a, b)) limb for limb.  Level l, D = l - 1, X the accumulators of the hybrid key switch (NTT form), P the
product of the special primes p_j, d the tensor term, A a plaintext added to c0, s_i a constant polynomial's value:
    z_j = [(iNTT(X_{p_j}) + floor(P/2)) (P/p_j)^-1]_{p_j}     t_i = sum_j z_j (P/p_j) - floor(P/2)  mod q_i
    c_D = s_D (iNTT_D(X_D + P (d_D + A_D)) - t_D) P^-1        u = [c_D + floor(q_D/2)]_{q_D},  u_i = (u mod q_i) - (floor(q_D/2) mod q_i)
    v_i = (s_i P^-1 t_i + u_i) q_D^-1                          r_i = s_i q_D^-1 (X_i P^-1 + d_i + A_i) - NTT_i(v_i)"""
import ctypes as C
from math import prod

import numpy as np
import pytest

from oracle.oracle import Ciphertext, Oracle, Plaintext, _p, splitmix_fill


def folded(o, a, b, A=None, s=None):
    ell, K, N, ks = a.ell, o.K, o.N, o.ks
    D, q, sp = ell - 1, [int(x) for x in o.primes], [int(x) for x in o.primes[o.K - o.ks :]]
    P, s = prod(sp), [1] * ell if s is None else [int(x) for x in s]
    t3 = o.tensor(a, b)
    X = np.zeros((2, ell + ks, N), dtype=np.uint64)  # the identity element: the digits of c2 as they are, times the relinearisation key
    o.L.orc_rotate_acc_hybrid(o.ctx, ell, _p(np.ascontiguousarray(t3[2])), C.c_uint32(1), _p(o.relin), _p(X))
    out = np.zeros((2, D, N), dtype=np.uint64)
    for p in range(2):
        d = t3[p].astype(object) + (A.astype(object) if (A is not None and p == 0) else 0)
        rho = o.ntt_inv(X[p, ell:], list(range(K - ks, K))).astype(object)
        T = sum((rho[j] + P // 2) * pow(P // sp[j], -1, sp[j]) % sp[j] * (P // sp[j]) for j in range(ks)) - P // 2  # an integer per coefficient
        row = ((X[p, D].astype(object) + P * d[D]) % q[D]).astype(np.uint64)
        cD = s[D] * (o.ntt_inv(row[None], [D])[0].astype(object) - T) * pow(P, -1, q[D]) % q[D]
        u = (cD + q[D] // 2) % q[D]
        for i in range(D):
            pinv, qinv = pow(P, -1, q[i]), pow(q[D], -1, q[i])
            v = ((s[i] * pinv * T + u % q[i] - (q[D] // 2) % q[i]) * qinv % q[i]).astype(np.uint64)
            out[p, i] = ((s[i] * qinv * (X[p, i].astype(object) * pinv + d[i]) - o.ntt_fwd(v[None], [i])[0].astype(object)) % q[i]).astype(np.uint64)
    return out


@pytest.mark.parametrize("widths,ks,alpha,ell", [(None, 3, 2, 2), (None, 3, 2, 3), ([60, 51, 51, 51, 60, 60], 2, 2, 3)])
def test_one_lifted_polynomial_per_kept_limb_equals_the_default_pair(widths, ks, alpha, ell):
    if widths:
        from dacapo_amd import ckks_boot as cb

        primes, v = [], {b: (1 << b) + 1 for b in widths}
        for b in widths:  # CoeffModulus::Create style per width class: scan down from 2^b in steps of 2N
            v[b] -= 2 << 10
            while not cb._is_prime(v[b]):
                v[b] -= 2 << 10
            primes.append(v[b])
    o = Oracle(10, 8, primes=primes if widths else None)
    o.set_hybrid(ks, alpha)
    o.keygen(seed=0x4845564D, galois_elts=[], relin=True)
    q = np.array(o.primes[:ell], dtype=np.uint64)[:, None]
    a, b, A = (np.stack([np.stack([splitmix_fill(sd + 7 * p + i, o.N) for i in range(ell)]) % q for p in range(2)]) for sd in (1, 99, 777))
    a, b = Ciphertext(a, 2.0**40), Ciphertext(b, 2.0**40)
    m = o.mul_relin(a, b)
    assert (folded(o, a, b) == o.rescale(m).data).all()
    S = o.encode(np.ones(o.slots), 2.0**20, ell)
    want = o.rescale(o.mul_plain(o.add_plain(m, Plaintext(A[0], m.scale)), S)).data
    assert (folded(o, a, b, A[0], S.data[:, 0]) == want).all()
