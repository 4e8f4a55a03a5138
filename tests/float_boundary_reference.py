"""Exact host reference of the integer <-> double boundary of opcode 10, the encoder's lift and the decoder's composition (Python integers,
Fractions and Python floats only: IEEE doubles, one rounding per operation, no contraction; no GPU and no project import).  A helper
module like sampler_reference.py, shared by tests/test_float_boundary_reference.py (CPU) and tests/test_gpu_float_boundary.py (GPU).

What the device computes (dacapo_amd/csrc/crt_device.hpp, hevm_vm.hip "opcode 10 on the device"):
    a_j   = crt_centered(residues of m_j)            Garner digits relative to those of floor(Q/2), summed in doubles
    r_0   = round(a_0 * ratio)                       round = half away from zero (std::round)
    r_N/2 = 0
    r_g   = round((a_g - a_{N-g}) * 0.5 * ratio),    r_{N-g} = -r_g                        0 < g < N/2
and then r (an integral double below 2^120) -> 128-bit integer -> residue of every target prime.  None of this needs an FFT to define.

Two zones (derived, not measured):
  * exact: every |m_j| < 2^52.  crt_centered returns float(m_j) itself (the high balanced digits cancel to an integer below 2^53 whatever
    the order of the sum, fused or not), a - b is exact, the rest is two multiplies and a round: the device must equal reencode_exact().
  * wide: |m| up to 2^118.  Every term of the digit sum carries at most 3 roundings (digit conversion, mdbl[k], product), the running sum
    at most ell, and sum |terms| <= 3 |m|, so |a - m| <= eps |m| with eps = 4 (ell + 2) 2^-53 (3 (ell + 2) to first order; the 4 absorbs
    the second order and the long double product behind mdbl).  reencode_bound() turns that into the tolerance on r."""
from __future__ import annotations

import math
from fractions import Fraction

U53 = Fraction(1, 1 << 53)   # unit round-off of a double


def rha(x: float) -> float:
    """std::round: to the nearest integer, halves away from zero (exact; no x + 0.5, which rounds 0.49999999999999994 up)"""
    if abs(x) >= 2.0**52 or x != x:
        return x
    t = float(int(x))                     # truncation, exact
    if abs(x - t) >= 0.5:                 # (x - t is exact: both below 2^52 with the same exponent or smaller)
        t += math.copysign(1.0, x)
    return t


def residues_of(x: int, primes) -> list:
    """canonical residues of a signed integer"""
    return [x % q for q in primes]


def compose_centered(residues, primes) -> int:
    """the integer m with m = residues[k] mod primes[k] and -floor(Q/2) <= m <= floor(Q/2) (Q odd: the range is symmetric)"""
    x, Q = 0, 1
    for r, q in zip(residues, primes):     # Garner: x + Q * ((r - x) / Q mod q)
        x += Q * (((int(r) - x) * pow(Q, -1, q)) % q)
        Q *= q
    h = Q >> 1
    return (x + h) % Q - h


def eps(ell: int) -> Fraction:
    """relative error bound of the device composition at ell primes (module docstring)"""
    return 4 * (ell + 2) * U53


def ratio_of(scale: float) -> float:
    """new_scale / old_scale of opcode 10: new_scale = 2^floor(log2 scale) (hevm_vm.hip boot_item), one division"""
    return 2.0 ** int(math.log2(scale)) / scale


def reencode_exact(m, ratio: float) -> list:
    """the re-encoded plaintext as the device evaluates it, from the exact coefficients m (Python ints, len N): valid as an equality
    in the exact zone"""
    N = len(m)
    r = [0] * N
    r[0] = int(rha(float(m[0]) * ratio))
    for g in range(1, N // 2):
        v = int(rha((float(m[g]) - float(m[N - g])) * 0.5 * ratio))
        r[g], r[N - g] = v, -v
    return r


def reencode_bound(m, ratio: float, ell: int):
    """(value, tolerance) per coefficient g <= N/2, as Fractions: value = ratio (m_g - m_{N-g}) / 2 (ratio m_0 at g = 0, 0 at N/2) and
    |r_dev - value| <= 1/2 + ratio (eps (|m_g| + |m_{N-g}|) / 2 + 3 * 2^-53 |m_g - m_{N-g}| / 2): the composition error of both operands,
    then three roundings (a - b, * ratio; * 0.5 is exact) and the round itself.  g = 0 is the same formula with m_{N-0} read as -m_0."""
    N, R, e = len(m), Fraction(ratio), eps(ell)
    out = [(R * m[0], Fraction(1, 2) + R * (e * abs(m[0]) + 3 * U53 * abs(m[0])))]
    for g in range(1, N // 2):
        a, b = m[g], m[N - g]
        out.append((R * (a - b) / 2, Fraction(1, 2) + R * (e * (abs(a) + abs(b)) / 2 + 3 * U53 * abs(a - b) / 2)))
    out.append((Fraction(0), Fraction(0)))
    return out


def constant_poly_limbs(m0: int, primes, N: int) -> list:
    """NTT-form limbs of the constant polynomial m0: every evaluation point gives m0 itself, so limb k is the constant array m0 mod q_k"""
    return [[m0 % q] * N for q in primes]


def is_prime(n: int) -> bool:
    """Miller-Rabin on the first twelve prime bases: deterministic below 3.3 * 10^24"""
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in bases:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in bases:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def chain(logN: int, widths) -> list:
    """one prime per entry of `widths`, CoeffModulus::Create style per width class: scan down from 2^b + 1 in steps of 2N, no repeats"""
    out, used = [], set()
    for b in widths:
        v = (1 << b) + 1
        while True:
            v -= 2 << logN
            if v not in used and is_prime(v):
                used.add(v)
                out.append(v)
                break
    return out


# ---- the device's composition in Python floats ------------------------------------------------------------------------------------------
def _fma(a: float, b: float, c: float) -> float:
    return float(Fraction(a) * Fraction(b) + Fraction(c))   # (Fraction -> float rounds to nearest even: one rounding)


def crt_tables(primes):
    """what HEVM::crt_tables uploads, as far as the double side goes: hdig = mixed-radix digits of floor(Q/2), mdbl[k] = double of
    q_0 ... q_{k-1} (here rounded once from the exact product; the device rounds a long double product -- inside eps)"""
    Q = 1
    for q in primes:
        Q *= q
    t, hdig, mdbl, prod = Q >> 1, [], [], 1
    for q in primes:
        hdig.append(t % q)
        t //= q
        mdbl.append(float(prod))
        prod *= q
    return hdig, mdbl


def crt_centered_model(residues, primes, fused: bool = False) -> float:
    """crt_device.hpp crt_centered: Garner digits v_k of (m + floor(Q/2)) mod Q on integers (the device's modular part is exact), then
    acc += double(v_k - hdig_k) * mdbl[k] from the top digit down; fused = the multiply-add contracted into one fma"""
    hdig, mdbl = crt_tables(primes)
    Q = 1
    for q in primes:
        Q *= q
    x = (compose_centered(residues, primes) + (Q >> 1)) % Q
    v = []
    for q in primes:
        v.append(x % q)
        x //= q
    acc = 0.0
    for k in range(len(primes) - 1, -1, -1):
        d = float(v[k] - hdig[k])
        acc = _fma(d, mdbl[k], acc) if fused else acc + d * mdbl[k]
    return acc
