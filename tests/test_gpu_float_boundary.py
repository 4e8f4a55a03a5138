"""GPU: where exact residues become doubles and come back -- opcode 10's composition, projection and rounding in its three launch forms,
the encoder's lift and the decoder's composition -- against tests/float_boundary_reference.py, an exact reference on Python integers.

Opcode 10 (a..c).  With the hook that makes encryptions of zero (0, 0), a register whose limbs are overwritten with c0 = NTT(residues of a
crafted integer polynomial m), c1 = 0 decrypts to m exactly whatever the secret, and the result of opcode 10 is (re-encoded plaintext, 0).
  * exact zone (every |m_j| < 2^52, or below Q_ell / 2 where that is smaller): every output limb == NTT(residues of reencode_exact(m, ratio));
  * wide zone (|m| up to 2^118): the output limbs, inverse-transformed on the CPU and composed over the target primes (Q_t > 2^121), lie
    within reencode_bound() of the rational value; r_{N-g} == -r_g and r_{N/2} == 0 exactly.
The launch forms: plan = 0 is reencode_kernel + lift_i128_kernel; plan = 1 from a source at 1 prime is f_boot_reencode_fcols (the VM
exports no counter of it: plan_boot_step takes it for every ell == 1 step of a ready plan, and the test asserts that the plan was ready and
that no instruction went through the one-at-a-time path); plan = 1 from two primes up is reencode_lift_batch_kernel.
Encoder (d): constants at power-of-two scales make coefficient 0 = round(c * scale) and all others 0 with no rounding in the FFT, so every
limb of the plaintext register is the constant array round(c * scale) mod q_k -- around 2^63, 2^64 and up to (2^53 - 1) 2^66.
Decoder (e): a constant polynomial m0 decodes to crt_centered(m0) / scale in every slot (the butterflies add exact zeros)."""
import ctypes
import math
import random
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import float_boundary_reference as fb  # noqa: E402
from gpu_helpers import _get_ct  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

LOGN = 12
N = 1 << LOGN
S40 = 2.0**40
SCALES = (S40, S40 * 1.37, 2.0**41 - 3 * 2.0**10)   # ratio 1, about 0.73, just above 0.5 (new scale = 2^40 for all three)


# ---- crafted polynomials ----------------------------------------------------------------------------------------------------------------
def _exact_zone_poly(bound, seed):
    """|m_j| <= bound (< 2^52): 0, +-1, +-bound, odd differences (ties at ratio 1), nonzero m_0 and m_{N/2}, small pairs, random fill"""
    rng, B = random.Random(seed), bound
    m = [rng.randrange(-B, B + 1) for _ in range(N)]
    for g in range(40, N // 2, 3):                      # many small pairs: a tie in every other one at ratio 1
        m[g], m[N - g] = rng.randrange(-9, 10), rng.randrange(-9, 10)
    pairs = [(0, 0), (1, 0), (0, 1), (-1, 0), (0, -1), (1, -1), (B, -B), (-B, B), (B, B), (B, B - 1), (B - 1, B), (B, -(B - 1)), (-B, B - 1),
             (7, 4), (-7, -2), (2, -1), (-2, 1), (B, 0), (0, B), (B - 1, 0), (3, 0), (-3, 0), (5, 0), (-5, 0)]
    for g, (a, b) in enumerate(pairs, start=1):
        m[g], m[N - g] = a, b
    m[0] = (B, -B, 1, -1, 3 - B, 12345)[seed % 6]
    m[N // 2] = 1 + 987654321 % B                        # must come out 0
    return m


def _wide_zone_poly(top_bits, seed):
    """53 <= bits of |m_g| <= top_bits (<= 118), swept by g: against 0, a small value, the opposite sign (|r| ~ |m|), a near-equal value
    (cancellation) and an unrelated magnitude; |r| around 2^63 and 2^64 at ratio 1 on the first pairs"""
    rng = random.Random(seed)
    m = [0] * N
    for g in range(1, N // 2):
        e = 53 + g % (top_bits - 52)
        a = rng.choice((-1, 1)) * rng.randrange(1 << (e - 1), 1 << e)
        e2 = rng.randrange(1, top_bits + 1)
        b = (0, rng.randrange(-(1 << 30), 1 << 30), -a + rng.randrange(1 << 20), a - rng.randrange(1 << (e // 2)),
             rng.choice((-1, 1)) * rng.randrange(1 << (e2 - 1), 1 << e2))[(g // (top_bits - 52)) % 5]
        m[g], m[N - g] = (a, b) if g % 2 else (b, a)
    if top_bits >= 66:
        edges = [(1 << 63) - (1 << 10), 1 << 63, (1 << 63) + (1 << 11), (1 << 64) - (1 << 11), 1 << 64, (1 << 64) + (1 << 12)]
        for g, t in enumerate(edges + [-t for t in edges], start=1):
            m[g], m[N - g] = (2 * t, 0) if g % 2 else (t, -t)
    m[0] = (-1) ** seed * ((1 << top_bits) - 12345)
    m[N // 2] = rng.randrange(1 << (top_bits - 1), 1 << top_bits)
    assert all(abs(x) <= 1 << top_bits for x in m)
    return m


def _residue_limbs(poly, primes):
    return np.array([[x % q for x in poly] for q in primes], dtype=np.uint64)


def _compose_columns(coef, primes):
    """compose_centered of every column of coef [t][N] (Garner with the inverses taken once)"""
    qs = [int(q) for q in primes]
    pre, Q = [], 1
    for q in qs:
        pre.append((Q, pow(Q, -1, q)))
        Q *= q
    h, rows, out = Q >> 1, [[int(v) for v in row] for row in coef], []
    for j in range(coef.shape[1]):
        x = 0
        for k, q in enumerate(qs):
            x += pre[k][0] * (((rows[k][j] - x) * pre[k][1]) % q)
        out.append((x + h) % Q - h)
    return out


# ---- opcode 10 through a tiny program -----------------------------------------------------------------------------------------------------
def _boot_program(ha, items, t):
    """items [(source primes, source scale)]: input i at its level and scale 2^40, relabelled with OP_SETSCALE where the scale is another,
    then opcode 10 to t primes.  Registers: i = input, n + i = relabelled view, 2n + i = result."""
    n, consts, ops = len(items), [], []
    for i, (ell, scale) in enumerate(items):
        src = i
        if scale != S40:
            consts.append([scale])
            ops.append((ha.OP_SETSCALE, n + i, i, len(consts) - 1))
            src = n + i
        ops.append((ha.OP_BOOTSTRAP, 2 * n + i, src, t))
    hv = ha.pack_hevm([40] * n, [ell for ell, _ in items], [40] * n, [t] * n, [2 * n + i for i in range(n)], 3 * n, 1,
                      max(ell for ell, _ in items), np.array(ops, dtype=np.uint16))
    return ha.pack_cst(consts), hv


def _inject(hevm, ll, o, reg, poly, ell):
    """overwrite register `reg` with (NTT(poly mod q_k), 0): layout [2][poly_stride / N][N]"""
    c = hevm.getCtxt(reg)
    assert c.level == ell and c.scale == S40
    full = np.zeros((2, c.poly_stride // N, N), dtype=np.uint64)
    full[0, :ell] = o.ntt_fwd(_residue_limbs(poly, o.primes[:ell]), list(range(ell)))
    ll.lib().dc_memcpy_h2d(c.data, full.ctypes.data, full.nbytes)


def _run_opcode10(primes, plan, items, t, seed=0x4845564D):
    """items [(zone, ell, scale, poly)] -> the VM's results checked against the reference, item by item"""
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    narrow = any(int(q).bit_length() != 60 for q in primes)
    hevm = runner.HEVM(seed=seed, logN=LOGN, num_primes=len(primes), primes=primes if narrow else None, vm_options={"plan": plan})
    o = Oracle(LOGN, len(primes), primes=primes)
    assert o.primes == list(primes) and hevm.K == len(primes) and hevm.N == N
    from dacapo_amd import LIB_PATH_GW

    assert (hevm.lw is runner.bind_vm_lib(LIB_PATH_GW)) == narrow   # the generic-width build for chains with narrow primes
    assert math.prod(primes[:t]) > 1 << 121
    hevm.lw.hevm_test_zero_encryption(hevm.vm, True)
    cst, hv = _boot_program(ha, [(ell, scale) for _, ell, scale, _ in items], t)
    hevm.load_mem(cst, hv)
    for i, (_, ell, _, poly) in enumerate(items):
        hevm.setInput(i, np.zeros(1))
        _inject(hevm, ll, o, i, poly, ell)
    hevm.run()
    st = hevm.stats()
    assert st["op_counts"][10] == len(items)
    plan_ready = hevm.lw.hevm_plan_lazy_groups(hevm.vm, None, 0) >= 0
    # plan = 1: every item ran as a step of the plan (ell == 1 steps take the fused form), none through HEVM::op_bootstrap, which times itself
    assert plan_ready == bool(plan) and (st["bootstrap_s"] == 0.0) == bool(plan)
    failures = []
    for i, (zone, ell, scale, poly) in enumerate(items):
        ratio = fb.ratio_of(scale)
        assert 0.5 < ratio <= 1.0
        out = _get_ct(hevm, ll, 2 * len(items) + i)
        assert out.ell == t and out.scale == S40
        assert not out.data[1].any()                      # c1 = 0: c0 is the re-encoded plaintext itself
        if zone == "exact":
            want = o.ntt_fwd(_residue_limbs(fb.reencode_exact(poly, ratio), primes[:t]), list(range(t)))
            bad = np.argwhere(out.data[0] != want)
            if len(bad):
                failures.append((zone, ell, ratio, "limbs differ", len(bad), bad[:4].tolist()))
            continue
        r = _compose_columns(o.ntt_inv(out.data[0], list(range(t))), primes[:t])
        if r[N // 2] != 0 or any(r[N - g] != -r[g] for g in range(1, N // 2)):
            failures.append((zone, ell, ratio, "not antisymmetric"))
        off = [(g, val) for g, (val, tol) in enumerate(fb.reencode_bound(poly, ratio, ell)) if abs(r[g] - val) > tol]
        if off:  # (the smallest magnitude that missed the bound: what a reduction that leaves its range shows first)
            lo = min(abs(val) for _, val in off)
            failures.append((zone, ell, ratio, "outside the bound", len(off), f"smallest |r| = 2^{math.log2(max(lo, 1)):.1f}", [g for g, _ in off[:6]]))
    hevm.close()
    assert not failures, failures


def _zone_items(primes, levels_exact, levels_wide, seed):
    items = []
    for ell in levels_exact:
        bound = min((1 << 52) - 1, math.prod(primes[:ell]) // 2 - 1)
        items += [("exact", ell, s, _exact_zone_poly(bound, seed + 10 * ell + k)) for k, s in enumerate(SCALES)]
    for ell in levels_wide:
        top = min(118, (math.prod(primes[:ell]) // 2).bit_length() - 1)
        items += [("wide", ell, s, _wide_zone_poly(top, seed + 10 * ell + k)) for k, s in enumerate(SCALES[:2])]
    return items


@pytest.mark.parametrize("plan", [1, 0])
def test_opcode10_exact_zone_equals_the_integer_reference(plan):
    """(a) 60-bit chain, sources at 1, 2, 3, 7 and 16 primes; three items per (ell, t) with three ratios in one program (a batch of three)"""
    primes = Oracle(LOGN, 17).primes
    _run_opcode10(primes, plan, _zone_items(primes, (1, 2, 3, 7, 16), (), seed=100), t=3)


@pytest.mark.parametrize("plan", [1, 0])
def test_opcode10_wide_zone_stays_within_the_derived_bound(plan):
    """(b) 60-bit chain, sources at 2, 3 and 16 primes, |m| swept from 2^53 to 2^118, both signs, |r| around 2^63 and 2^64"""
    primes = Oracle(LOGN, 17).primes
    _run_opcode10(primes, plan, _zone_items(primes, (), (2, 3, 16), seed=200), t=3)


@pytest.mark.parametrize("plan", [1, 0])
@pytest.mark.parametrize("widths", [[46] * 5, [51] * 5, [55, 60, 45, 51, 58, 60]], ids=["46x5", "51x5", "mixed"])
def test_opcode10_on_the_generic_width_build(widths, plan):
    """(c) both zones on narrow and mixed chains, sources at 1, 2 and 3 primes; from 3 primes the wide zone reaches |r| ~ 2^118, far beyond
    2^(2b+4) of a 46- or 51-bit prime -- where the lift of the batched form must not reduce as if the integer were a product of residues"""
    primes = fb.chain(LOGN, widths)
    from dacapo_amd import ckks_boot as cb

    assert all(cb._is_prime(q) for q in primes)
    _run_opcode10(primes, plan, _zone_items(primes, (1, 2, 3), (2, 3), seed=300 + widths[0]), t=3)


# ---- (d) the encoder's lift ---------------------------------------------------------------------------------------------------------------
def _lift_values():
    big = [2.0**63 - 2.0**10, 2.0**63, 2.0**63 + 2.0**11, 2.0**64] + [float((1 << 53) - 1) * 2.0**k for k in (10, 11, 12, 63, 64, 66)]
    assert big[0] == math.nextafter(2.0**63, 0.0)
    vals = big + [-v for v in big] + [2.0**40 + 0.5, -(2.0**40) - 0.5, 2.0**52 + 1.0]   # (the halves: ties, away from zero)
    assert all(abs(v) < 2.0**120 for v in vals)
    return vals


@pytest.mark.parametrize("host_encoder", [0, 1])
@pytest.mark.parametrize("bits", [60, 51])
def test_encoder_lift_of_constants_around_the_branch_edges(bits, host_encoder):
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    K, level, sb = 5, 4, 60
    vals = _lift_values()
    consts = [[v / 2.0**sb] for v in vals]                # exact: a power-of-two scaling
    assert all(Fraction(c[0]) * (1 << sb) == Fraction(v) for c, v in zip(consts, vals))
    ops = [(ha.OP_ENCODE, i, i, (level << 10) + sb) for i in range(len(vals))] + [(ha.OP_NEGATE, 1, 0, 0)]
    hv = ha.pack_hevm([40], [level], [40], [level], [1], 2, len(vals), level, np.array(ops, dtype=np.uint16))
    opts = {"host_encoder": host_encoder}
    if bits != 60:
        opts["prime_bits"] = bits
    hevm = runner.HEVM(seed=21, logN=LOGN, num_primes=K, vm_options=opts)
    primes = Oracle(LOGN, K, bit_size=bits).primes
    assert [int(q).bit_length() for q in primes] == [bits] * K
    hevm.load_mem(ha.pack_cst(consts), hv)                # all constants at one level: the device encoder sees them as one batch
    for i, v in enumerate(vals):
        lvl, sc = ctypes.c_int32(), ctypes.c_double()
        p = hevm.lw.hevm_plain(hevm.vm, i, ctypes.byref(lvl), ctypes.byref(sc))
        assert p and lvl.value == level and sc.value == 2.0**sb
        got = ll.read_device(p, (level, N))
        want = int(fb.rha(v))
        for k in range(level):
            assert (got[k] == np.uint64(want % primes[k])).all(), (v, k, int(got[k][0]), want % primes[k])
    hevm.close()


# ---- (e) the decoder's composition ----------------------------------------------------------------------------------------------------------
def _decode_constant(hevm, ll, primes, reg, ell, m0):
    c = hevm.getCtxt(reg)
    assert c.level == ell and c.scale == S40
    c0 = np.array(fb.constant_poly_limbs(m0, primes[:ell], N), dtype=np.uint64)
    ll.lib().dc_memcpy_h2d(c.data, c0.ctypes.data, c0.nbytes)      # (c1 is zero since setInput: the zero-encryption hook is on)
    out = np.zeros(N // 2)
    hevm.lw.decrypt(hevm.vm, reg, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return out


def test_decoder_composition_of_constant_polynomials():
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    K, levels = 19, (2, 8, 16, 17, 18)
    hevm = runner.HEVM(seed=33, logN=LOGN, num_primes=K)
    primes = Oracle(LOGN, K).primes
    hevm.lw.hevm_test_zero_encryption(hevm.vm, True)
    n = len(levels)
    hv = ha.pack_hevm([40] * n, list(levels), [40], [levels[0]], [n], n + 1, 1, max(levels), np.array([(ha.OP_NEGATE, n, 0, 0)], dtype=np.uint16))
    hevm.load_mem(ha.pack_cst([]), hv)
    for i in range(n):
        hevm.setInput(i, np.zeros(1))
        assert not _get_ct(hevm, ll, i).data.any()
    rng = random.Random(5)
    inv_scale = 1.0 / S40
    shared = {}   # m0 below Q_16 / 2 -> what the 16-limb register decoded it to
    for reg, ell in enumerate(levels):
        comp = min(ell, 16)                                # HEVM::decrypt composes the first 16 limbs of a deeper register
        h = math.prod(primes[:comp]) // 2
        exact = [0, 1, -1, (1 << 52) - 1, 1 - (1 << 52), rng.randrange(1 << 52), -rng.randrange(1 << 52)]
        wide = [h, -h, h - 1, 1 - h, 1 << 53, -(1 << 53) - 1]
        for e in np.linspace(54, h.bit_length() - 1, 8).astype(int):
            wide.append(rng.choice((-1, 1)) * rng.randrange(1 << (int(e) - 1), 1 << int(e)))
        for m0 in (sorted(shared) if ell > 16 else exact + wide):
            slots = _decode_constant(hevm, ll, primes, reg, ell, m0)
            assert (slots == slots[0]).all(), (ell, m0)
            got = Fraction(float(slots[0]))
            if abs(m0) < 1 << 52:
                assert slots[0] == float(m0) * inv_scale, (ell, m0)
            else:
                q = Fraction(m0, 1 << 40)
                assert abs(got - q) <= fb.eps(comp) * abs(q) + fb.U53 * abs(q), (ell, m0, float(slots[0]))
            if ell == 16:
                shared[m0] = float(slots[0])
            elif ell > 16:
                assert float(slots[0]) == shared[m0], (ell, m0)   # the first-16-limbs rule: limbs 17 and 18 change nothing
    hevm.close()
