"""CPU: the reference of the integer <-> double boundary against itself (tests/float_boundary_reference.py), an integer model of the four
"integral double -> 128-bit integer -> residue" lifts of the device code with every accumulator range-checked (next to the models of
tests/test_modarith_model.py, whose multiply and fold it reuses), and a Python-float model of crt_centered held to the bound the GPU tests
apply (tests/test_gpu_float_boundary.py).

The lifts (each a hand copy of the same two branches, |x| < 2^63 and beyond):
    enc_round_lift_kernel (encoder.hip), store_i128 + lift_i128_kernel (hevm_vm.hip), residue_of_double (crt_device.hpp): reduce128_any
    store_residues (hevm_vm.hip, the batched opcode 10 from sources at two primes up): reduce128_any as well -- it used to call
    canon(reduce128_lazy(h, l)) directly, whose precondition T < 2^(2b+4) a 119-bit integer breaks on a narrow prime:
    test_lazy_reduction_alone_leaves_its_range_on_narrow_primes keeps that finding executable.
Which of the two reductions a lift's model runs is read from the lift's source (device_reducer): the models follow the code."""
import math
import random
import re
from fractions import Fraction
from pathlib import Path

import pytest

import float_boundary_reference as fb
from test_modarith_model import M32, M64, chain_primes, fold_b, mulmod_lazy, reduce_words


# ---- the reference against itself -------------------------------------------------------------------------------------------------------
CHAINS = {"60": fb.chain(12, [60] * 16), "51": fb.chain(12, [51] * 16), "46": fb.chain(12, [46] * 5),
          "mixed": fb.chain(12, [55, 60, 45, 51, 58, 60] * 3)[:16]}


def _edge_and_random_ints(Q, rng, count=40):
    h = Q >> 1
    xs = [0, 1, -1, 2, -2, h, -h, h - 1, 1 - h, (1 << 52) - 1, 1 - (1 << 52), 1 << 52, 1 << 53, (1 << 53) + 1, -(1 << 63), (1 << 64) + 12345]
    for _ in range(count):
        e = rng.randrange(1, max(2, h.bit_length()))
        xs.append(rng.choice((-1, 1)) * rng.randrange(1 << (e - 1), 1 << e))
    return [x for x in xs if abs(x) <= h]


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_composition_round_trips_against_residues(name):
    rng = random.Random(len(name) + 7)
    for ell in (1, 2, 3, 5, len(CHAINS[name])):
        primes = CHAINS[name][:ell]
        Q = math.prod(primes)
        for x in _edge_and_random_ints(Q, rng):
            res = fb.residues_of(x, primes)
            assert all(0 <= r < q for r, q in zip(res, primes))
            assert fb.compose_centered(res, primes) == x
        assert fb.compose_centered(fb.residues_of(Q // 2 + 1, primes), primes) == -(Q // 2)   # the range is symmetric: Q is odd
    assert fb.constant_poly_limbs(-3, CHAINS[name][:2], 4) == [[q - 3] * 4 for q in CHAINS[name][:2]]


def test_ties_round_away_from_zero_and_round_is_odd():
    for x, want in ((0.5, 1.0), (-0.5, -1.0), (1.5, 2.0), (-1.5, -2.0), (2.5, 3.0), (-2.5, -3.0), (0.49999999999999994, 0.0),
                    (-0.49999999999999994, 0.0), (2.0**52 - 0.5, 2.0**52), (2.0**52 + 1, 2.0**52 + 1), (-(2.0**53) - 2, -(2.0**53) - 2),
                    (2.0**118, 2.0**118), (0.0, 0.0), (7.0, 7.0), (-7.25, -7.0), (7.75, 8.0)):
        assert fb.rha(x) == want and fb.rha(-x) == -want
    rng = random.Random(3)
    for _ in range(2000):
        x = rng.uniform(-1, 1) * 2.0 ** rng.randrange(0, 56)
        r = fb.rha(x)
        assert r == int(r) and abs(Fraction(r) - Fraction(x)) <= Fraction(1, 2) and fb.rha(-x) == -r
        if abs(Fraction(r) - Fraction(x)) == Fraction(1, 2):
            assert abs(r) > abs(x)


def test_reencode_exact_is_antisymmetric_and_ties_show_at_ratio_one():
    rng = random.Random(11)
    N = 64
    m = [rng.randrange(-(1 << 52) + 1, 1 << 52) for _ in range(N)]
    m[3], m[N - 3] = 7, 4            # difference 3: 1.5 -> 2
    m[5], m[N - 5] = -7, -2          # difference -5: -2.5 -> -3
    m[N // 2] = 12345                # must come out 0
    for ratio in (1.0, fb.ratio_of(2.0**40 * 1.37), fb.ratio_of(2.0**41 - 1)):
        assert 0.5 < ratio <= 1.0
        r = fb.reencode_exact(m, ratio)
        assert r[N // 2] == 0 and all(r[N - g] == -r[g] for g in range(1, N // 2))
        assert r[0] == int(fb.rha(float(m[0]) * ratio))
        for g, (val, tol) in enumerate(fb.reencode_bound(m, ratio, 2)):
            assert abs(r[g] - val) <= tol
    r = fb.reencode_exact(m, 1.0)
    assert (r[3], r[N - 3], r[5], r[N - 5], r[0]) == (2, -2, -3, 3, m[0])


# ---- the four lifts, on integers --------------------------------------------------------------------------------------------------------
def canon(x, b, d):
    q = (1 << b) - d
    r = fold_b(x, b, d)
    assert r < 2 * q, "one conditional subtraction would not finish"
    return r - q if r >= q else r


def reduce128_lazy(h, l, b, d):
    return reduce_words(h, l >> 32, l & M32, b, d)


def reduce128_any(h, l, b, d):
    q = (1 << b) - d
    if b < 60:  # fw_narrow: (hi mod q) (2^64 mod q) + (lo mod q)
        r63 = canon(1 << 63, b, d)
        r64 = r63 + r63 - q if r63 + r63 >= q else r63 + r63
        a, c = canon(mulmod_lazy(r64, canon(h, b, d), b, d), b, d), canon(l, b, d)
        return a + c - q if a + c >= q else a + c
    return canon(reduce128_lazy(h, l, b, d), b, d)


def reduce128_lazy_canon(h, l, b, d):
    return canon(reduce128_lazy(h, l, b, d), b, d)


def double_to_hl(a):
    """the two branches every lift repeats: a >= 0 integral, below 2^120 -> (h, l) with h 2^64 + l = a"""
    assert a >= 0.0 and a == math.floor(a) and a < 2.0**120
    if a < 2.0**63:
        l, h = int(a), 0
    else:
        fr, e = math.frexp(a)                 # a = fr 2^e, fr in [0.5, 1)
        mant = int(math.ldexp(fr, 53))
        sh = e - 53
        assert 1 << 52 <= mant < 1 << 53 and 11 <= sh <= 67
        if sh < 64:                           # both shift counts are in 1..63: defined in C++
            assert 0 < 64 - sh < 64
            l, h = (mant << sh) & M64, mant >> (64 - sh)
        else:
            assert 0 <= sh - 64 < 64
            l, h = 0, mant << (sh - 64)
        assert h <= M64
    assert (h << 64) | l == int(a)
    return h, l


def _negmod(r, q):
    return q - r if r else 0


def lift_enc_round(x, b, d, reduce):          # encoder.hip enc_round_lift_kernel, crt_device.hpp residue_of_double: the same statements
    h, l = double_to_hl(abs(x))
    r = reduce(h, l, b, d)
    return _negmod(r, (1 << b) - d) if x < 0.0 else r


def lift_store_i128(x, b, d, reduce):         # hevm_vm.hip store_i128 (two's complement out) + lift_i128_kernel (and back)
    h, l = double_to_hl(abs(x))
    if x < 0.0:
        l = (~l + 1) & M64
        h = (~h + (l == 0)) & M64
    neg = h >> 63 != 0
    assert neg == (x < 0.0)
    if neg:
        l = (~l + 1) & M64
        h = (~h + (l == 0)) & M64
    r = reduce(h, l, b, d)
    return _negmod(r, (1 << b) - d) if neg else r


def lift_store_residues(x, b, d, reduce, flip=False):   # hevm_vm.hip store_residues
    neg = (x < 0.0) != flip
    h, l = double_to_hl(abs(x))
    r = reduce(h, l, b, d)
    return _negmod(r, (1 << b) - d) if neg else r


CSRC = Path(__file__).resolve().parent.parent / "dacapo_amd" / "csrc"
# lift -> (source file, the function that reduces, its model)
LIFTS = {"enc_round_lift": ("encoder.hip", "enc_round_lift_kernel", lift_enc_round),
         "residue_of_double": ("crt_device.hpp", "residue_of_double", lift_enc_round),
         "store_i128": ("hevm_vm.hip", "lift_i128_kernel", lift_store_i128),
         "store_residues": ("hevm_vm.hip", "store_residues", lift_store_residues)}


def device_reducer(name):
    """the reduction the device code of this lift calls, read from its source, as the model of it: the models follow the code, so a lift
    that goes back to canon(reduce128_lazy(..)) alone fails test_every_lift_stays_in_range_and_gives_the_residue on the narrow primes"""
    file, fn, _ = LIFTS[name]
    src = (CSRC / file).read_text()
    body = src[re.search(r"\b" + fn + r"\(", src).start():]
    body = body[: body.index("\n}\n")]
    if "reduce128_any(" in body:
        return reduce128_any
    assert re.search(r"canon\(reduce128_lazy\(", body), f"{fn}: no known reduction in its body"
    return reduce128_lazy_canon


BD = [(60, (1 << 60) - chain_primes()[0]), (60, (1 << 28) - 1), (60, 1), (51, (1 << 28) - 1), (51, (1 << 26) + 12345), (46, (1 << 27) + 99),
      (45, (1 << 26) - 1000)]   # the (b, d) pairs of test_modarith_model.py
REAL_BD = [(b, (1 << b) - fb.chain(12, [b])[0]) for b in (46, 51, 55)]   # first primes of the chains the GPU tests run on (d ~ 2^13)


def _lift_operands(rng):
    """integral doubles below 2^120: every exponent 0..119 with random 53-bit mantissas, and the branch edges"""
    xs = [0.0, 1.0, 2.0**53 - 1, 2.0**63 - 2.0**10, 2.0**63, 2.0**63 + 2.0**11, 2.0**64 - 2.0**11, 2.0**64, 2.0**64 + 2.0**12,
          float((1 << 53) - 1) * 2.0**66, float((1 << 52) + 1) * 2.0**67, 2.0**119]
    for sh in (11, 12, 62, 63, 64, 65, 66, 67):
        xs += [float(1 << 52) * 2.0**sh, float((1 << 53) - 1) * 2.0**sh, float(rng.randrange(1 << 52, 1 << 53)) * 2.0**sh]
    for e in range(120):
        for _ in range(6):
            mant = rng.randrange(1 << 52, 1 << 53)
            xs.append(float(mant >> (52 - e)) if e < 52 else float(mant) * 2.0 ** (e - 52))
    assert all(x < 2.0**120 for x in xs)
    return xs


@pytest.mark.parametrize("lift", sorted(LIFTS))
@pytest.mark.parametrize("b,d", BD + REAL_BD)
def test_every_lift_stays_in_range_and_gives_the_residue(b, d, lift):
    q = (1 << b) - d
    rng = random.Random(b * 7919 + d)
    model, reduce = LIFTS[lift][2], device_reducer(lift)
    for a in _lift_operands(rng):
        for x in (a, -a):
            assert model(x, b, d, reduce) == int(x) % q
            if lift == "store_residues":
                assert model(x, b, d, reduce, flip=True) == (-int(x)) % q


def _first_exponent_out_of_range(b, d, reduce):
    """smallest e such that some integral double in [2^e, 2^(e+1)) trips a range assertion of the model (or gives a wrong residue)"""
    q = (1 << b) - d
    for e in range(120):
        for x in (2.0**e, float((1 << 53) - 1) * 2.0 ** (e - 52)):
            if x != math.floor(x):
                continue
            try:
                if lift_store_residues(x, b, d, reduce) != int(x) % q:
                    return e
            except AssertionError:
                return e
    return None


def test_lazy_reduction_alone_leaves_its_range_on_narrow_primes():
    """The finding behind store_residues calling reduce128_any: canon(reduce128_lazy(h, l)) assumes T < 2^(2b+4).  A 60-bit prime keeps
    every |x| < 2^120 inside it; a narrower one does not -- from which magnitude on depends on d = 2^b - q as well (the step
    (Bv >> (b - 32)) must fit a word, and Bv = H1 d): a few bits above 2^(2b+4) for the widest d the context accepts, and only where
    hi = T >> 64 reaches 2^b (T >= 2^(64+b)) for the small d of CoeffModulus-style primes.  reduce128_any stays in range on all of them
    (test_every_lift_stays_in_range_and_gives_the_residue)."""
    for b, d in BD:
        first = _first_exponent_out_of_range(b, d, reduce128_lazy_canon)
        if b == 60:
            assert first is None
        else:
            assert first is not None and 2 * b + 4 <= first <= 64 + b, (b, d, first)
    assert [_first_exponent_out_of_range(b, d, reduce128_lazy_canon) for b, d in BD[3:]] == [106, 107, 97, 96]
    assert [_first_exponent_out_of_range(b, d, reduce128_lazy_canon) for b, d in REAL_BD] == [105, 115, 119]
    for b, d in BD + REAL_BD:
        assert _first_exponent_out_of_range(b, d, reduce128_any) is None


# ---- crt_centered in Python floats ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_balanced_digits_of_half_the_modulus(name):
    """hdig_k == (q_k - 1) / 2 at every level: v_k - hdig_k is the BALANCED digit, |.| <= (q_k - 1) / 2, which is what sum |terms| <= 3 |m|
    of the error bound rests on"""
    for ell in range(1, len(CHAINS[name]) + 1):
        hdig, mdbl = fb.crt_tables(CHAINS[name][:ell])
        assert hdig == [(q - 1) // 2 for q in CHAINS[name][:ell]]
        assert mdbl[0] == 1.0 and all(Fraction(mdbl[k]) == Fraction(float(math.prod(CHAINS[name][:k]))) for k in range(ell))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_composition_in_doubles_meets_the_stated_bound(name, fused):
    """|crt_centered(m) - m| <= eps(ell) |m| for ell = 1..16 (fused multiply-add or not), float(m) itself below q_0 / 2 (one digit, one
    conversion), and m itself below 2^52 on every chain, also where q_0 is narrower than that (the exact zone of the GPU tests)"""
    rng = random.Random(len(name) * 31 + fused)
    for ell in range(1, len(CHAINS[name]) + 1):
        primes = CHAINS[name][:ell]
        Q = math.prod(primes)
        for m in _edge_and_random_ints(Q, rng, count=25):
            a = fb.crt_centered_model(fb.residues_of(m, primes), primes, fused=fused)
            err = abs(Fraction(a) - m)
            assert err <= fb.eps(ell) * abs(m), (ell, m, a)
            if abs(m) < primes[0] // 2:
                assert a == float(m)
            if abs(m) < 1 << 52:
                assert a == m
