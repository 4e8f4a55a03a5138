#!/usr/bin/env python3
"""A/B of the grouped-digit base conversions on the matrix cores against the vector kernels, per key shape (option hyb_mfma when the context is
created; csrc/hybrid_ks.hip hyb_conv_mfma_kernel / hyb_conv_mfma_wide_kernel), one box, ONE process, warm-up first:
    python tools/legs/hyb_wide_digits_ab.py [--rounds 5] [--calls 10] [--logn 17] [--level 31] [--shapes 8:9,11:12,16:16] [--out FILE]
Per shape alpha:ksp, under hyb_fuse = 2: one dc_ct_rotate_hop and one dc_ct_mul_relin at level --level, device events on the stream.  Three arms
alternate -- vector A, matrix cores, vector B (two contexts with hyb_mfma = 0: their difference is the off/off spread) --, --rounds rounds of
--calls calls each; mean and spread (min .. max) of the rounds, us per call.  The arms' results are compared limb for limb before anything is
timed.  Nothing is fixed in advance: a difference within the off/off spread is recorded as no difference."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s + "\n")


def shape_leg(logN, ell, alpha, ks, rounds, calls):
    import numpy as np

    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    L, N, K = ll.lib(), 1 << logN, ell + ks
    arms = {}
    for name, mfma in (("vector A", 0), ("matrix", 1), ("vector B", 0)):
        with runner.options(hyb_mfma=mfma):
            arms[name] = ll.Context(logN, K, special=ks, alpha=alpha)
        assert L.dc_context_conv_matrix_cores(arms[name].h, ell) == mfma
    ctx0 = arms["matrix"]
    rng = np.random.default_rng(1)
    q = np.array(ctx0.primes, dtype=np.uint64)
    dkey = ll.DeviceBuffer.from_host(rng.integers(0, 1 << 59, size=(ctx0.key_digits, 2, K, N), dtype=np.uint64) % q[None, None, :, None])  # timing only
    a, b = (ll.DeviceBuffer.from_host(rng.integers(0, 1 << 59, size=(2, ell, N), dtype=np.uint64) % q[None, :ell, None]) for _ in range(2))
    out = {n: ll.DeviceBuffer((2, ell, N)) for n in arms}
    st = ell * N
    e0, e1 = L.dc_event_create(), L.dc_event_create()
    ops = {"dc_ct_rotate_hop": lambda n: L.dc_ct_rotate_hop(arms[n].h, out[n].ptr, st, a.ptr, st, 3, dkey.ptr, ell, None),
           "dc_ct_mul_relin": lambda n: L.dc_ct_mul_relin(arms[n].h, out[n].ptr, st, a.ptr, st, b.ptr, st, dkey.ptr, ell, None)}
    with runner.options(hyb_fuse=2):
        for op, fn in ops.items():
            for n in arms:  # warm-up
                for _ in range(3):
                    fn(n)
            L.dc_stream_sync(None)
            ref = out["matrix"].to_host()
            assert all((out[n].to_host() == ref).all() for n in arms), op
            t = {n: [] for n in arms}
            for _ in range(rounds):
                for n in arms:
                    L.dc_event_record(e0, None)
                    for _ in range(calls):
                        fn(n)
                    L.dc_event_record(e1, None)
                    t[n].append(L.dc_event_elapsed_ms(e0, e1) * 1e3 / calls)
            m = {n: sum(v) / len(v) for n, v in t.items()}
            off = 0.5 * (m["vector A"] + m["vector B"])
            say(f"N=2^{logN} l={ell} digits of {alpha} under {ks} special primes {op:17s}: " + "   ".join(
                f"{n} {m[n]:8.1f} us ({min(t[n]):.1f} .. {max(t[n]):.1f})" for n in arms)
                + f"   matrix - vector {m['matrix'] - off:+7.1f} us   off/off spread {abs(m['vector A'] - m['vector B']):5.1f} us")


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return args[args.index(name) + 1] if name in args else default

    rounds, calls, logn, ell = int(opt("--rounds", 5)), int(opt("--calls", 10)), int(opt("--logn", 17)), int(opt("--level", 31))
    for shape in opt("--shapes", "8:9,11:12,16:16").split(","):
        alpha, ks = (int(x) for x in shape.split(":"))
        shape_leg(logn, ell, alpha, ks, rounds, calls)
    if "--out" in args:
        Path(opt("--out", None)).write_text("".join(LINES))


if __name__ == "__main__":
    main()
