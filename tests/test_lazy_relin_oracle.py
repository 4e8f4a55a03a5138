"""Lazy relinearisation restated on the CPU oracle: relin(sum_k s_k a_k (x) b_k) with ONE key switch (dc_ct_mul_sum_relin's definition:
T = sum_k s_k Oracle.tensor(a_k, b_k) by poly_add / poly_sub, then Oracle.keyswitch(T2, relin, T0, T1)) decrypts to sum_k s_k x_k y_k.

The yardstick is the default composition on the same inputs: n x mul_relin, then negate / add.  One key switch's noise replaces n, so the lazy
result's error should be no larger; the bound is 2 x the default's maximum slot error, the factor covering the spread of a maximum over 2 048
slots.  N = 2^12, 5 primes, level 3, three products with signs + - +."""
import numpy as np

from oracle.oracle import Ciphertext


def test_one_key_switch_for_a_signed_sum_of_products(oracle_mid):
    o = oracle_mid
    ell, scale, signs = 3, 2.0**40, [1, -1, 1]
    rng = np.random.default_rng(20261020)
    xs = [rng.uniform(-1, 1, o.slots) for _ in signs]
    ys = [rng.uniform(-1, 1, o.slots) for _ in signs]
    cx = [o.encrypt(o.encode(v, scale, ell)) for v in xs]
    cy = [o.encrypt(o.encode(v, scale, ell)) for v in ys]
    clear = sum(s * x * y for s, x, y in zip(signs, xs, ys))

    T = np.zeros((3, ell, o.N), dtype=np.uint64)
    for s, a, b in zip(signs, cx, cy):
        t = o.tensor(a, b)
        T = np.stack([(o.poly_add if s > 0 else o.poly_sub)(T[p], t[p]) for p in range(3)])
    c0, c1 = T[0].copy(), T[1].copy()
    o.keyswitch(T[2], o.relin, c0, c1)
    lazy = o.decode(o.decrypt(Ciphertext(np.stack([c0, c1]), scale * scale)))

    acc = None
    for s, a, b in zip(signs, cx, cy):
        p = o.mul_relin(a, b)
        p = p if s > 0 else o.negate(p)
        acc = p if acc is None else o.add(acc, p)
    default = o.decode(o.decrypt(acc))

    err_lazy = float(np.abs(lazy[: o.slots] - clear).max())
    err_default = float(np.abs(default[: o.slots] - clear).max())
    assert err_default < 1e-6, err_default  # (the yardstick itself decrypts to the clear result)
    assert err_lazy <= 2 * err_default, f"lazy {err_lazy:.3e} against default {err_default:.3e} (bound 2 x)"
    # with one product and sign + the definition IS mul_relin: the anchor to SEAL's rounding
    t = o.tensor(cx[0], cy[0])
    c0, c1 = t[0].copy(), t[1].copy()
    o.keyswitch(t[2], o.relin, c0, c1)
    assert (np.stack([c0, c1]) == o.mul_relin(cx[0], cy[0]).data).all()
