"""The exact reference of the error statistics (dc_poly_error_stats, dacapo_amd/noise.py): residues are lifted to centred Python integers
over ALL their limbs, and the sums are exact rationals.  The CPU test (test_noise_reference.py) holds it against the closed forms on the
oracle; the GPU tests (test_gpu_noise.py) hold the device against it."""
from fractions import Fraction

import numpy as np


def lift(coef, primes):
    """coef [ell][N] coefficient-domain residues -> object array of the N integers in (-Q/2, Q/2], Q = prod primes (Garner, Python ints)"""
    coef = np.asarray(coef)
    x = coef[0].astype(object)
    Q = int(primes[0])
    for i in range(1, len(primes)):
        q = int(primes[i])
        inv = pow(Q % q, -1, q)
        x = x + Q * (((coef[i].astype(object) - x) * inv) % q)
        Q *= q
    return np.where(x > Q // 2, x - Q, x)  # Q is odd: x <= (Q - 1) / 2 stays


def stats_of(values, m=1, inconsistent=0):
    """the record of integers D_j with divisor m: exact"""
    vals = [int(v) for v in values]
    return {"sum_sq": Fraction(sum(v * v for v in vals), m * m), "sum": Fraction(sum(vals), m), "max_abs": max(abs(v) for v in vals),
            "inconsistent": int(inconsistent)}


def error_stats(o, got, want, ell, lift_prime=-1):
    """dc_poly_error_stats for ONE polynomial on the oracle `o`: got / want [>= ell][N] NTT-form residues (want None = 0), D = m got - want
    limb by limb, the oracle's inverse transform, then: the value of every coefficient is the centred lift of limbs 0 and 1 (limb 0 at
    ell = 1), and a coefficient is inconsistent when the centred lift over ALL limbs is another integer."""
    primes = [int(q) for q in o.primes[:ell]]
    m = 1 if lift_prime < 0 else int(o.primes[lift_prime])
    D = np.zeros((ell, o.N), dtype=np.uint64)
    for i, q in enumerate(primes):
        d = (m % q) * np.asarray(got[i]).astype(object)
        if want is not None:
            d = d - np.asarray(want[i]).astype(object)
        D[i] = (d % q).astype(np.uint64)
    coef = o.ntt_inv(D, list(range(ell)))
    two, full = lift(coef[:2], primes[:2]), lift(coef, primes)
    return stats_of(two, m, int(np.count_nonzero(two != full)))


def secret_weight(o):
    """non-zero coefficients of the oracle's secret key"""
    return int(np.count_nonzero(o.ntt_inv(o.sk[:1], [0])[0]))


def close(got, want, rel=1e-9):
    """a double against an exact rational"""
    want = Fraction(want)
    return abs(Fraction(got) - want) <= Fraction(rel) * abs(want)
