"""Noise an operation adds, measured on the device in the unit of the reference compiler's noiseTable
(lib/Dialect/Earth/IR/EarthDialect.cpp:154-178 reads it, ErrorEstimator.cpp:54-59 sums it):

    noise = (N/2) . mean over coefficients of e_j^2

where e is the error polynomial the operation adds -- the phase c0 + c1 s of its result minus the exact function of its operands'
phases -- as centred integers, unscaled.  (N/2) mean e^2 is the variance of the real part of one slot of e.

The phases of all streams come from one launch (hevm_phase_batch), the expected polynomial from the exact plaintext-side device ops
(dc_galois_ntt, dc_poly_mul, dc_poly_add), and the statistics of got - want from dc_poly_error_stats: nothing but the final records
crosses to the host.  A VM created with any options can be measured: hoisted hops, grouped digits, sparse secrets."""
from __future__ import annotations

import ctypes

import numpy as np

from . import hevm_asm as ha
from . import lowlevel as ll

KEY_NOISE_VARIANCE = 10.5  # the 21-21 centred binomial of the key generator (tests/sampler_reference.py)
OPS = ("rotate", "rescale", "mul")


def phase(hevm, reg: int, streams, first_stream: int = 0, pad_limbs: int = 0) -> ll.DeviceBuffer:
    """c0 + c1 s of cipher register `reg` of `streams` streams from first_stream on: a DeviceBuffer [streams][level][N], NTT form.
    pad_limbs: that many zero limbs after each stream's `level` ([streams][level + pad_limbs][N])."""
    count = int(streams)
    limbs = int(hevm.getCtxt(reg).level) + pad_limbs
    out = ll.DeviceBuffer((count, limbs, hevm.N))
    if pad_limbs:  # (the fill runs on the default stream, the phases on the VM's own: the fill must have finished first)
        ll.lib().dc_memset(out.ptr, 0, out.nbytes)
        ll.lib().dc_device_sync()
    level = hevm.lw.hevm_phase_batch(hevm.vm, reg, ctypes.c_void_p(out.ptr), limbs * hevm.N, first_stream, count)
    assert level + pad_limbs == limbs
    return out


def measure(hevm, build, want, level: int, samples: int, inputs: int = 1, lift_prime: int = -1, pad_limbs: int = 0, seed: int = 1,
            loop: bool = False, observe=None) -> dict:
    """The noise of the program `build(b, xs)` emits on a hevm_asm.Builder -- xs: its `inputs` arguments at `level` primes and scale
    2^40, the return value its result -- over `samples` encryptions of uniform [-1, 1] messages, run ONCE on `samples` streams.  The
    inputs' phases are taken before run() and the result's after; want(ctx, phases) -> (polynomials, stride in words) forms the expected
    polynomial of every sample from the list of input phases [samples][level][N] with ctx's exact ops (ctx: the VM's
    lowlevel.Context).  lift_prime: dc_poly_error_stats' multiplier, for results that are a division (rescale); pad_limbs: zero limbs
    appended to the result's phase, so that it can be held against an operand of more limbs (the multiplier is 0 on a padded limb).
    loop: one stream per run(), `samples` runs -- for VMs created under option plan = 0, whose loop takes one stream.
    observe(first, count): called after each run(), while the registers of samples first .. first + count - 1 are still in place.
    Returns {noise, coeff_var, coeff_mean, max_abs, inconsistent, samples, level, per_sample}: noise = sum_sq / (2 samples)."""
    b = ha.Builder(slots=hevm.slots, init_level=level, shadow=False)
    xs = [b.input(None) for _ in range(inputs)]
    b.output(build(b, xs))
    cst, hv, _ = b.assemble()
    ctx = ll.Context.of_vm(hevm)
    msgs = np.random.default_rng(seed).uniform(-1.0, 1.0, (inputs, samples, hevm.slots))
    hevm.set_streams(1 if loop else samples)
    hevm.load_mem(cst, hv)
    res = hevm.getResIdx(0)
    stats, out_level = [], None
    for first, count in ([(s, 1) for s in range(samples)] if loop else [(0, samples)]):
        for i in range(inputs):
            hevm.setInputs(i, msgs[i, first : first + count])
        phases = [phase(hevm, i, count) for i in range(inputs)]
        hevm.run()
        got = phase(hevm, res, count, pad_limbs=pad_limbs)
        out_level = got.shape[1] - pad_limbs
        exp, stride = want(ctx, phases)
        stats += ctx.error_stats(got, exp, got.shape[1], count, lift_prime, want_stride=stride)
        if observe is not None:
            observe(first, count)
    n = samples * hevm.N
    sum_sq, total = sum(s.sum_sq for s in stats), sum(s.sum for s in stats)
    return {"noise": sum_sq / (2.0 * samples), "coeff_var": sum_sq / n - (total / n) ** 2, "coeff_mean": total / n,
            "max_abs": max(s.max_abs for s in stats), "inconsistent": sum(int(s.inconsistent) for s in stats), "samples": samples,
            "level": out_level,
            "per_sample": [{"sum_sq": s.sum_sq, "sum": s.sum, "max_abs": s.max_abs, "inconsistent": int(s.inconsistent)} for s in stats]}


def _raw(b, opcode, level, x, rhs=0, rhs_is_value=False):
    """one instruction without the builder's scale bookkeeping (a rescale of a 2^40 input, a product kept at its level)"""
    out = b._new(level, x.scale_bits, None)
    b._emit(opcode, out, x, rhs, rhs_is_value)
    return out


def op_noise(hevm, op: str, level: int, samples: int, loop: bool = False, seed: int = 1, observe=None) -> dict:
    """measure() of one operation at `level` primes:
    rotate  -- one hop, offset 1, against galois(phase)
    rescale -- level -> level - 1 (level >= 2), against the operand through lift_prime: e = (q_last . out - in) / q_last, the result padded
               with a zero limb and held against ALL the operand's limbs: q_last . out - in is then lifted from two limbs even at
               level 2, where it exceeds q_0 / 2
    mul     -- ct x ct + relinearise, against phase_a . phase_b"""
    if op == "rotate":
        def want(ctx, ph):
            count = ph[0].shape[0]
            out = ll.DeviceBuffer((count, level, ctx.N))
            ctx.galois_ntt(out, level * ctx.N, ph[0], level * ctx.N, ctx.elt_from_step(1), count, level)
            return out, level * ctx.N

        return measure(hevm, lambda b, xs: b.rotate(xs[0], 1), want, level, samples, seed=seed, loop=loop, observe=observe)
    if op == "rescale":
        if level < 2:
            raise ValueError("a rescale needs two primes")
        return measure(hevm, lambda b, xs: _raw(b, ha.OP_RESCALE, level - 1, xs[0]), lambda ctx, ph: (ph[0], level * ctx.N), level, samples,
                       lift_prime=level - 1, pad_limbs=1, seed=seed, loop=loop, observe=observe)
    if op == "mul":
        def want(ctx, ph):
            count = ph[0].shape[0]
            out = ll.DeviceBuffer((count, level, ctx.N))
            for k in range(count):
                ctx.poly_mul(out.at(k * level * ctx.N), ph[0].at(k * level * ctx.N), ph[1].at(k * level * ctx.N), level)
            return out, level * ctx.N

        return measure(hevm, lambda b, xs: _raw(b, ha.OP_MULCC, level, xs[0], xs[1].id, True), want, level, samples, inputs=2, seed=seed,
                       loop=loop, observe=observe)
    raise ValueError(f"op {op!r} is not one of {OPS}")


def closed_form(op: str, primes, ell: int, N: int, h: float) -> float:
    """What the operation's noise should be, in measure()'s unit.  primes: the key-level chain, the last one special (SEAL-layout keys);
    ell: the operand's primes; h: the secret's non-zero coefficients (2N/3 on average for the default ternary secret).
    rescale: (N/2)(1 + h)/12 -- the rounding tau_0 + tau_1 s, tau uniform in an interval of length 1.
    rotate, mul: the key switch's (N/2)(N . 10.5 . sum_{j < ell} q_j^2 / (3 P^2) + (1 + h)/12): ell digits, non-negative residues of q_j
    (E d^2 = q_j^2 / 3), each times a key noise of variance 10.5 over N coefficients, divided by P -- and that division's rounding."""
    rounding = (1.0 + h) / 12.0
    if op == "rescale":
        return N / 2.0 * rounding
    if op in ("rotate", "mul"):
        P = float(primes[-1])
        return N / 2.0 * (N * KEY_NOISE_VARIANCE * sum(float(q) ** 2 for q in primes[:ell]) / (3.0 * P * P) + rounding)
    raise ValueError(f"op {op!r} is not one of {OPS}")
