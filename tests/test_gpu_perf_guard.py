"""Perf regression guard for the launch-shape options (csrc/options.hpp: a dozen thresholds tuned on boxes that differ by +-1.5 %; each forced
shape has a parity test, this is the timing side).  With every option at its default it times the three figures the rounds are judged on -- a
rotation hop at 13 primes, config 3 (ct x ct + relinearise, N = 2^16, 24 + 1 primes) and one run() of the headline program -- and holds each to
within 5 % of the figure committed for the round (tests/golden/perf_guard.json, written by THIS file's own measurement code on the round's
final build: `python tests/test_gpu_perf_guard.py --record gpurun_out/perf_guard.json` on the GPU box).  Boxes are not identical: the device-to-device copy rate is measured first and the test is SKIPPED when it
is more than 3 % BELOW that of the box the committed figures came from -- a slower box is not a regression.  A box that copies faster (boxes of
the same model differ by 10 %) runs the checks against the same committed figures: it has no excuse to be slower.  Faster than the committed
figure never fails."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
GUARD = ROOT / "tests" / "golden" / "perf_guard.json"
TOLERANCE, BOX_TOLERANCE = 0.05, 0.03


def _copy_gbs(ll, rounds=3, iters=10):
    L = ll.lib()
    n = 4096 * 32768
    a, b = ll.DeviceBuffer((n,)), ll.DeviceBuffer((n,))
    L.dc_memset(a.ptr, 1, a.nbytes)
    e0, e1 = L.dc_event_create(), L.dc_event_create()
    best = 0.0
    for _ in range(rounds):
        L.dc_memcpy_d2d(b.ptr, a.ptr, a.nbytes, None)
        L.dc_event_record(e0, None)
        for _ in range(iters):
            L.dc_memcpy_d2d(b.ptr, a.ptr, a.nbytes, None)
        L.dc_event_record(e1, None)
        best = max(best, 2.0 * a.nbytes / (L.dc_event_elapsed_ms(e0, e1) / iters * 1e-3) / 1e9)
    return best


@pytest.fixture(scope="module")
def guard():
    if not GUARD.exists():
        pytest.skip("no committed figures (tests/golden/perf_guard.json)")
    g = json.loads(GUARD.read_text())
    sys.path.insert(0, str(ROOT))
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    runner.reinit_lw().hevm_reset_options()  # defaults, whatever an earlier module left behind
    for L in runner._option_libs():
        L.hevm_reset_options()
    gbs = _copy_gbs(ll)
    if gbs / g["copy_kernel_gbs"] - 1.0 < -BOX_TOLERANCE:
        pytest.skip(f"this box copies at {gbs:.0f} GB/s, the committed figures' box at {g['copy_kernel_gbs']:.0f}: more than 3 % slower")
    return g


def _hop13_us(ll):
    import bench

    return min(bench.per_op_leg(ll, iters=50, only="rotate_hop")["rotate_hop"]["us"] for _ in range(3))


def _cfg3_us(ll):
    import bench

    return min(bench.cfg3_leg(ll, iters=10, grouped=False)["us"] for _ in range(3))


def _headline(runner):
    """(ms per run() of the headline program: best of three rounds of five, rms of the decrypted logits against the torch model's)"""
    import time

    from dacapo_amd import hevm_asm as ha

    fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
    vm = runner.HEVM(fresh=True, logN=15, num_primes=14)
    vm.load_mem(fx["cst"], fx["hevm"])
    vm.setInput(0, fx["packed"])
    for _ in range(3):
        vm.run()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(5):
            vm.run()
        best = min(best, (time.perf_counter() - t0) / 5 * 1e3)
    out = vm.getOutput()[0]
    vm.close()
    return best, float(np.sqrt(np.mean((out[:10] * 32 - fx["torch_result"]) ** 2)))


def _check(name, measured, committed):
    assert measured <= committed * (1.0 + TOLERANCE), f"{name}: {measured:.2f} against the committed {committed:.2f} (+{(measured / committed - 1) * 100:.1f} %)"


def test_rotation_hop_at_13_primes(guard):
    from dacapo_amd import lowlevel as ll

    _check("rotation hop at 13 primes, us", _hop13_us(ll), guard["hop13_us"])


def test_config3_mul_relin(guard):
    from dacapo_amd import lowlevel as ll

    _check("config 3 (N = 2^16, 24 + 1 primes), us", _cfg3_us(ll), guard["cfg3_us"])


def test_headline_run(guard):
    from dacapo_amd import runner

    ms, rms = _headline(runner)
    assert rms < 2e-3
    _check("headline run(), ms", ms, guard["headline_ms"])


if __name__ == "__main__":  # python tests/test_gpu_perf_guard.py --record <out.json> [round]: the figures of THIS box and build, by the code above
    sys.path.insert(0, str(ROOT))
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    assert len(sys.argv) >= 3 and sys.argv[1] == "--record", __doc__
    rec = {"round": sys.argv[3] if len(sys.argv) > 3 else "r06", "source": "tests/test_gpu_perf_guard.py --record (same code as the checks)",
           "copy_kernel_gbs": round(_copy_gbs(ll), 1), "hop13_us": _hop13_us(ll), "cfg3_us": _cfg3_us(ll)}
    rec["headline_ms"], rec["headline_rms_vs_torch"] = _headline(runner)
    rec["headline_ms"] = round(rec["headline_ms"], 3)
    Path(sys.argv[2]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[2]).write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
