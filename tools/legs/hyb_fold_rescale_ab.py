#!/usr/bin/env python3
"""A/B of a rescale folded into the grouped-digit multiply's mod-down (option hyb_fold_rescale, dc_ct_mul_relin_rescale on a grouped-digit
context; csrc/hybrid_fused.hip hybf_mul_relin_rescale_tail), one box, ONE process, warm-up first:
    python tools/legs/hyb_fold_rescale_ab.py [--rounds 5] [--calls 20] [--logn 17] [--steps 3] [--skip-run] [--out profiles/hyb_fold_rescale_ab.txt]
  (a) per op, device events on the stream: dc_ct_mul_relin followed by dc_ct_rescale against one dc_ct_mul_relin_rescale at N = 2^17, 31 + 9 primes,
4 digits of 8 (config 4's key shape), l = 3, 8, 14, under hyb_fuse = 1 and 2.  The two forms alternate, --rounds rounds of --calls calls each;
mean and spread (min .. max) of the rounds, us per call.  The results of the two forms are compared limb for limb before anything is timed.
  (b) config 4 (resnet20_nt16.b14, its default and its real_msg = True lowering), wall clock around run(): three VMs one after the other --
      option off, on, off again (the rotation keys of one fill a third of HBM) --, a warm-up run and --steps timed ones each.  Merged pairs
      (hevm_last_run_fold_rescale_stats) and the rms against the committed torch logits.  The two off VMs give the off/off spread.
No speed-up is fixed in advance: a difference within the off/off spread is recorded as no difference."""
import gzip
import time
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s + "\n")


def op_leg(logN, K, ks, alpha, levels, rounds, calls):
    import numpy as np

    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    L, N = ll.lib(), 1 << logN
    ctx = ll.Context(logN, K, special=ks, alpha=alpha)
    rng = np.random.default_rng(1)
    q = np.array(ctx.primes, dtype=np.uint64)
    dkey = ll.DeviceBuffer.from_host(rng.integers(0, 1 << 59, size=(ctx.key_digits, 2, K, N), dtype=np.uint64) % q[None, None, :, None])  # timing only
    e0, e1 = L.dc_event_create(), L.dc_event_create()
    for fuse in (1, 2):
        for ell in levels:
            a, b = (ll.DeviceBuffer.from_host(rng.integers(0, 1 << 59, size=(2, ell, N), dtype=np.uint64) % q[None, :ell, None]) for _ in range(2))
            prod, two, one = ll.DeviceBuffer((2, ell, N)), ll.DeviceBuffer((2, ell - 1, N)), ll.DeviceBuffer((2, ell - 1, N))
            st, st1 = ell * N, (ell - 1) * N

            def separate():
                L.dc_ct_mul_relin(ctx.h, prod.ptr, st, a.ptr, st, b.ptr, st, dkey.ptr, ell, None)
                L.dc_ct_rescale(ctx.h, two.ptr, st1, prod.ptr, st, ell, None)

            def folded():
                L.dc_ct_mul_relin_rescale(ctx.h, one.ptr, st1, a.ptr, st, b.ptr, st, dkey.ptr, None, None, ell, None)

            def timed(fn):
                L.dc_event_record(e0, None)
                for _ in range(calls):
                    fn()
                L.dc_event_record(e1, None)
                return L.dc_event_elapsed_ms(e0, e1) * 1e3 / calls

            with runner.options(hyb_fuse=fuse):
                for fn in (separate, folded):  # warm-up
                    for _ in range(3):
                        fn()
                L.dc_stream_sync(None)
                assert (one.to_host() == two.to_host()).all()
                t = {"separate": [], "folded": []}
                for _ in range(rounds):
                    t["separate"].append(timed(separate))
                    t["folded"].append(timed(folded))
            m = {k: sum(v) / len(v) for k, v in t.items()}
            say(f"op N=2^{logN} {K - ks}+{ks} primes alpha={alpha} hyb_fuse={fuse} l={ell:2d}: dc_ct_mul_relin + dc_ct_rescale {m['separate']:8.1f} us "
                f"({min(t['separate']):.1f} .. {max(t['separate']):.1f})   dc_ct_mul_relin_rescale {m['folded']:8.1f} us "
                f"({min(t['folded']):.1f} .. {max(t['folded']):.1f})   difference {m['folded'] - m['separate']:+7.1f} us   ratio {m['folded'] / m['separate']:5.3f}")


def run_leg(real_msg, steps, ks=9, alpha=8):
    import numpy as np

    from dacapo_amd import ckks_boot as cb
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import runner

    golden = ROOT / "tests" / "golden" / "resnet20_nt16"
    fx = ha.read_fixture(golden)
    K = 14 + cb.boot_levels() + ks
    hv, cst = cb.lower_bootstraps(gzip.open(str(golden) + ".b14.hevm.gz").read(), fx["cst"], 17, K, msg_bits=1, ks=ks, real_msg=real_msg)
    mean, tag = {}, f"config 4 real_msg={int(real_msg)}"
    for name, fold in (("off A", 0), ("on", 1), ("off B", 0)):
        vm = runner.HEVM(fresh=True, logN=17, num_primes=K, ks_special=ks, ks_alpha=alpha, vm_options={"secret_hw": 64, "hyb_fold_rescale": fold})
        vm.addRotationKeys(cb.rotation_offsets(hv))
        vm.load_mem(cst, hv)
        vm.setInput(0, fx["packed"])
        vm.run()  # warm-up
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            vm.run()
            ts.append((time.perf_counter() - t0) * 1e3)
        rms = float(np.sqrt(np.mean((vm.getOutput()[0][:10] * 32 - fx["torch_result"]) ** 2)))
        mean[name] = sum(ts) / len(ts)
        say(f"run {tag} hyb_fold_rescale {name:5s}: mean {mean[name]:8.1f} ms ({min(ts):.1f} .. {max(ts):.1f})   pairs {vm.fold_rescale_stats():4d}   "
            f"rms vs torch logits {rms:.3e}")
        vm.close()
    say(f"run {tag} on - off {mean['on'] - 0.5 * (mean['off A'] + mean['off B']):+7.1f} ms   off/off spread {abs(mean['off A'] - mean['off B']):6.1f} ms")


def main():
    args = sys.argv[1:]

    def opt(name, default):
        return args[args.index(name) + 1] if name in args else default

    rounds, calls, logn, out = int(opt("--rounds", 5)), int(opt("--calls", 20)), int(opt("--logn", 17)), opt("--out", None)
    op_leg(logn, 40, 9, 8, (3, 8, 14), rounds, calls)
    if "--skip-run" not in args:
        for real_msg in (False, True):
            run_leg(real_msg, int(opt("--steps", 3)))
    if out:
        Path(out).write_text("".join(LINES))


if __name__ == "__main__":
    main()
