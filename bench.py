#!/usr/bin/env python3
"""bench.py -- HEVM hot-path benchmark on MI355X (contract: see the task statement / DESIGN.md "Measurement").

step      = one run() of the ResNet-20 HEVM program (nt = 2^14 slots, N = 2^15, 14 x 60-bit primes: the parameters
            SEAL_HEVM.cpp:39-53 hard-codes) on ciphertexts already resident in HBM; the timed region is run() only,
            exactly what examples/tests/ResNet.py:109-111 times.  The program is the op stream of the reference's own
            examples/benchmarks/ResNet.py (traced through python/poly, lowered by hevm_asm's lazy-rescale policy) with
            the real BN-folded weights, committed as data under tests/golden/resnet20.* ; the decrypted logits are
            compared with the torch model's (rms_vs_torch, what examples/tests/ResNet.py prints).
            --program shaped selects the older synthetic program with the same op mix.
value     = NTT-equivalents per second over the whole job (all ranks): (l+1)(l+2) per key switch, 2l per rescale
            (SURVEY.md 3.4 / BASELINE.md 1) divided by the max-over-ranks wall time of K steps.
roofline  = the dominant kernel pair (forward negacyclic NTT = COLS phase + ROWS phase launch) on a 4096-limb batch,
            timed with HIP events on the launch stream; algorithmic bytes = 2 * N * 8 per limb.
cpu_baseline = the CPU oracle (C restatement of SEAL 4.0's algorithms, 1 thread like the reference) on a bounded
            prefix of the same program, rank 0, N = 1 only.
Launch: python bench.py [--gpus N --steps K --warmup W]   (N > 1: via torch.distributed.run, one rank per GPU).
A plain run measures the headline only: set-up, W warm-up steps, K timed steps, the result line.  roofline, cpu_baseline, the
decrypted-error check, config 4 and every other leg run only with --full.  --dump-outputs DIR writes the decrypted result of the
last timed step (what getOutput() hands a caller) as DIR/<name>.npy.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

KEY_SEED = 0x4845564D  # --dry-run only (stand-in key buffers expanded with numpy): a real run generates keys from the OS's randomness (hevm_init_fresh)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
PROF = "r06"  # the round whose profiles/ records this file reads (each is used only when its lib_sha256 is the library being timed)


def ntt_equivalents(stats_or_counts):
    return stats_or_counts["ntts"]


def roofline_leg(ll, ctx, limbs=4096, iters=10):
    """forward NTT over `limbs` limbs of N = 2^15 as dc_ntt_forward launches it: the single-crossing kernel (round 3; one launch)"""
    L = ll.lib()
    N = ctx.N
    buf = ll.DeviceBuffer((limbs, N))
    host = (np.arange(limbs * N, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(5)
    L.dc_memcpy_h2d(buf.ptr, host.ctypes.data, host.nbytes)
    e0, e1 = L.dc_event_create(), L.dc_event_create()

    def timed(variant):
        L.dc_event_record(e0, None)
        for _ in range(iters):
            ctx.ntt(buf, limbs, prime_base=0, prime_period=ctx.K, variant=variant)
        L.dc_event_record(e1, None)
        return L.dc_event_elapsed_ms(e0, e1) / iters

    # The leg follows a stretch of host work (the VM teardown, a context build): the first ~20 ms of kernels run before the clocks are back
    # up (measured: the same launch 10-14 % slower when timed first).  So: warm up with 20 launches, then three alternating rounds of the
    # library's choice (None: the single-crossing kernel) and the round-2 transform (0), best of three each.
    for _ in range(20):
        ctx.ntt(buf, limbs, prime_base=0, prime_period=ctx.K)
    rounds = [(timed(None), timed(0)) for _ in range(3)]
    # `achieved` / `frac` come from the MEAN over the rounds (30 launches); the best round is reported beside it, not instead of it
    ms, two_ms = sum(r[0] for r in rounds) / len(rounds), sum(r[1] for r in rounds) / len(rounds)
    best_ms = min(r[0] for r in rounds)
    alg_bytes = 2.0 * limbs * N * 8
    gbs = alg_bytes / (ms * 1e-3) / 1e9
    # what a plain device-to-device copy of the same buffer reaches on this GPU (read + write), for scale
    dst = ll.DeviceBuffer((limbs, N))
    L.dc_memcpy_d2d(dst.ptr, buf.ptr, buf.nbytes, None)
    L.dc_event_record(e0, None)
    for _ in range(iters):
        L.dc_memcpy_d2d(dst.ptr, buf.ptr, buf.nbytes, None)
    L.dc_event_record(e1, None)
    copy_gbs = 2.0 * buf.nbytes / (L.dc_event_elapsed_ms(e0, e1) / iters * 1e-3) / 1e9
    del buf, dst
    # HBM bytes per launch: rocprofv3 --pmc passes cannot run inside this process (they need their own runs with the program directly
    # after `--`, tools/legs/ntt_variant_only.py).  profiles/<round>_ntt_hbm_traffic.json holds FETCH_SIZE (x2, the gfx950 correction) + WRITE_SIZE
    # for the same launches; it is reported only when it was collected on exactly this build of the library.
    traffic, traffic_source = None, "not collected for this build (recipe: profiles/README.md, `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE`)"
    tf = ROOT / "profiles" / f"{PROF}_ntt_hbm_traffic.json"
    if tf.exists() and limbs == 4096 and N == 32768:
        rec = json.loads(tf.read_text())
        if rec.get("lib_sha256") == lib_sha256():
            traffic, traffic_source = rec.get("forward_ntt_hbm_bytes"), f"profiles/{PROF}_ntt_hbm_traffic.json (PMC passes on this build)"
        else:
            traffic_source = f"profiles/{PROF}_ntt_hbm_traffic.json was collected on another build of the library: not reported"
    floor_us = alg_bytes / (copy_gbs * 1e9) * 1e6
    # what actually bounds the kernel: the vector ALUs' issue rate (profiles/r03_ntt_full.txt).  The counters come from their own rocprofv3
    # --pmc run (tools/summarize/ntt_valu.py) and are reported only for exactly this build of the library.
    valu = {"source": "not collected for this build (recipe: tools/collect_profiles.sh B4b, tools/summarize/ntt_valu.py)"}
    vf = ROOT / "profiles" / f"{PROF}_ntt_valu.json"
    if vf.exists() and limbs == 4096 and N == 32768:
        rec = json.loads(vf.read_text())
        if rec.get("lib_sha256") == lib_sha256():
            k = next((v for n, v in rec.get("kernels", {}).items() if n.startswith("ntt_full15_kernel<false")), None)
            if k:
                valu = {"source": f"profiles/{PROF}_ntt_valu.json (rocprofv3 --pmc on this build)",
                        "valu_instructions_per_wave_per_limb": k.get("valu_instructions_per_wave_per_limb"),
                        "simd_valu_busy_frac": k.get("simd_valu_busy_frac"),
                        "clock_ghz_if_counter_sums_8_xcds": k.get("clock_ghz_if_counter_sums_8_xcds")}
        else:
            valu = {"source": f"profiles/{PROF}_ntt_valu.json was collected on another build of the library: not reported"}
    return {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
            "traffic": traffic, "traffic_source": traffic_source,
            "kernel": "ntt_full15_kernel<fwd> (a 1024-thread workgroup owns a limb, one HBM crossing; persistent grid of one workgroup per CU; "
                      "dacapo_amd/csrc/ntt_full.hip)",
            "launch": {"limbs": limbs, "N": N, "algorithmic_bytes": alg_bytes, "avg_us": round(ms * 1e3, 2),
                       "ntt_per_s": round(limbs / (ms * 1e-3)),
                       "timing": "HIP events around 10 back-to-back launches; 20 warm-up launches, then three alternating rounds of the library's "
                                 "choice and the two-launch transform: avg_us / achieved / frac are the MEAN of the three rounds",
                       "rounds_us": [[round(a * 1e3, 1), round(b * 1e3, 1)] for a, b in rounds],
                       "best_round": {"avg_us": round(best_ms * 1e3, 2), "frac": round(alg_bytes / (best_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}},
            # (no measured figure is hard-coded here: the counters of THIS build are in `valu`, reported only when their lib_sha256 matches;
            # the ablations behind the statement are a record of round 3's build of the same kernel source)
            "limiting_resource": "VALU issue and the twiddles' vector-memory path (60-bit modular butterflies on 32-bit ALUs); the HBM fraction is "
                                 "what that arithmetic leaves.  Evidence: `valu` (this build's counters, when collected) and the ablation record "
                                 "profiles/r03_ntt_full.txt (round 3's build of the same kernel: loads / stores / both removed)",
            "valu": valu,
            "single_crossing": {"hbm_crossings_per_limb": 1, "copy_floor_us": round(floor_us, 1), "frac_of_copy_floor": round(floor_us / (ms * 1e3), 4),
                                "source": "profiles/r03_ntt_full.txt (round 3's record of this kernel: ablations, exchanges 2 and 3 through LDS, the "
                                          "modular multiply's carries, persistent grid walking prime by prime, twiddle pairs in passes A and B, "
                                          "variants that lost)"},
            "two_launch_transform": {"avg_us": round(two_ms * 1e3, 2), "frac": round(alg_bytes / (two_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                     "note": "round 2's COLS + ROWS launch pair on the same buffer (still used below 640 limbs forward / 2048 "
                                             "inverse, and for N != 2^15)"},
            "copy_kernel_gbs": round(copy_gbs, 1), "frac_of_copy": round(gbs / copy_gbs, 4)}


def real_bootstrap_leg(ll, runner, steps=3, resnet=True):
    """Real CKKS bootstrapping (dacapo_amd/ckks_boot.py; the reference's HEaaN runtime's `bootstrap`, HEAAN_HEVM.cpp:386-399, for which
    its SEAL runtime's opcode 10 is a stand-in): one ciphertext 1 prime -> 3 primes at the reference's two ring sizes, and the ResNet-20
    trace with a real bootstrap at every bootstrap site (lowered here from tests/golden/resnet20.*).  20 x 60-bit primes, secret of Hamming weight 64,
    direct Galois keys for the offsets used.  Parity: unpinned (HEaaN is closed); what is checked is the decrypted result."""
    from dacapo_amd import ckks_boot as cb
    from dacapo_amd import hevm_asm as ha

    sparse = {"secret_hw": 64}
    KB = 3 + cb.boot_levels() + 1
    out = {"parameters": f"{KB} x 60-bit primes ({KB - 1} data + 1 special), secret Hamming weight 64, r = 5 double angles, 4 + 10 + 3 levels",
           "reference": "profiled_HEAAN_GPU.json earth.bootstrap_single: 0.29-0.46 s at N = 2^17 on HEaaN (its GPU unstated)", "single": []}
    for logN in (15, 17):
        K, cst, hv, offs, _ = cb.single_bootstrap_program(logN)
        hevm = runner.HEVM(fresh=True, logN=logN, num_primes=K, vm_options=sparse)
        hevm.addRotationKeys(offs)
        hevm.load_mem(cst, hv)
        msg = np.random.default_rng(3).uniform(-1, 1, hevm.slots)
        hevm.setInput(0, msg)
        hevm.run()
        t0 = time.perf_counter()
        for _ in range(steps):
            hevm.run()
        dt = (time.perf_counter() - t0) / steps
        err = np.abs(hevm.getOutput()[0] - msg)
        st = hevm.stats()
        from dacapo_amd import progstats

        pst = progstats.walk(hv, logN, direct_keys=True)
        sec = (f"below 128-bit (N = 2^15, log2(QP) = {60 * K}, secret Hamming weight 64; the HE standard allows 881 bits at this N): "
               "timing / accuracy demonstration only") if logN == 15 else \
              f"N = 2^17, log2(QP) = {60 * K}, h = 64: inside the 128-bit range for this ring"
        out["single"].append({"N": 1 << logN, "security": sec, "ms": round(dt * 1e3, 2), "instructions": int(len(ha.unpack_hevm(hv)["ops"])),
                              "algorithmic_bytes": pst["algorithmic_bytes"], "achieved_gbs": round(pst["algorithmic_bytes"] / dt / 1e9, 1),
                              "frac_of_hbm_peak": round(pst["algorithmic_bytes"] / dt / 1e9 / HBM_PEAK_GBS, 4),
                              "key_switches": st["keyswitches"], "ntt_equivalents": st["ntts"], "ntt_per_s": round(st["ntts"] / dt),
                              "max_error": float(err.max()), "rms_error": float(np.sqrt(np.mean(err**2))),
                              "precision_bits": round(float(-np.log2(err.max())), 1)})
        hevm.close()  # hevm_destroy: the next VM gets this one's HBM back
    if resnet:
        fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
        t0 = time.time()
        fx["hevm"], fx["cst"] = cb.lower_bootstraps(fx["hevm"], fx["cst"], 15, KB, msg_bits=4)  # every opcode 10 -> real bootstrapping
        t_lower = time.time() - t0
        hevm = runner.HEVM(fresh=True, logN=15, num_primes=KB, vm_options=sparse)
        hevm.addRotationKeys(cb.rotation_offsets(fx["hevm"]))
        hevm.load_mem(fx["cst"], fx["hevm"])
        hevm.setInput(0, fx["packed"])
        t0 = time.perf_counter()
        hevm.run()
        dt = time.perf_counter() - t0
        o, st = hevm.getOutput()[0], hevm.stats()
        ops = ha.unpack_hevm(fx["hevm"])["ops"]
        out["resnet20_with_real_bootstraps"] = {
            "program": "the headline program, every opcode 10 lowered to ModRaise/CoeffToSlot/EvalMod/SlotToCoeff by ckks_boot.lower_bootstraps",
            "security": f"below 128-bit (N = 2^15, log2(QP) = {60 * KB}, h = 64): timing / accuracy demonstration only; config 4 (N = 2^17) is the "
                        "parameter set inside the standard's range",
            "lowering_s": round(t_lower, 1),
            "instructions": int(len(ops)), "real_bootstraps": int((ops[:, 0] == ha.OP_MODRAISE).sum()), "run_s": round(dt, 3),
            "key_switches": st["keyswitches"], "ntt_equivalents": st["ntts"], "ntt_per_s": round(st["ntts"] / dt),
            "rms_vs_torch": float(np.sqrt(np.mean((o[:10] * 32 - fx["torch_result"]) ** 2))),
            "rms_vs_plaintext_evaluation": float(np.sqrt(np.mean((o - fx["expected"]) ** 2)))}
        hevm.close()
    return out


def streams_leg(hevm, cst, hv, image, ntts_per_image, alg_bytes_per_image, steps=3, counts=(1, 2, 4, 8, 16)):
    """Throughput mode (hevm_set_streams): S independent ciphertext streams of the SAME program in one VM -- every batched step carries the
    items of all S images, so the launch chain that bounds one image (~5 300 dependent launches of 4-30 us) is shared by S of them.  This is
    the regime BASELINE config 5 runs in (streams x GPUs); the headline keeps S = 1 like the reference (one image per run())."""
    out = {"what": "S independent images of the headline program per run() in one VM (extension hevm_set_streams); value of the headline = the S = 1 row's regime",
           "rows": []}
    for S in counts:
        hevm.set_streams(S)
        hevm.load_mem(cst, hv)
        for sidx in range(S):
            hevm.select_stream(sidx)
            hevm.setInput(0, image if sidx == 0 else np.roll(image, 13 * sidx))
        hevm.run()
        t0 = time.perf_counter()
        for _ in range(steps):
            hevm.run()
        dt = (time.perf_counter() - t0) / steps
        gbs = S * alg_bytes_per_image / dt / 1e9
        out["rows"].append({"streams": S, "ms_per_run": round(dt * 1e3, 3), "ms_per_image": round(dt * 1e3 / S, 3),
                            "ntt_per_s": round(S * ntts_per_image / dt), "step_algorithmic_gbs": round(gbs, 1),
                            "step_algorithmic_frac": round(gbs / HBM_PEAK_GBS, 4)})
    hevm.set_streams(1)
    return out


def lib_sha256():
    import hashlib

    from dacapo_amd import LIB_PATH

    return hashlib.sha256(Path(LIB_PATH).read_bytes()).hexdigest()


def per_op_leg(ll, ell=13, iters=20, only=None):
    """the three expensive opcodes alone at the reference's top level (13 primes, N = 2^15), next to the reference's own
    per-op table for SEAL on a CPU (profiled_SEAL_CPU.json:10-45); algorithmic bytes per SURVEY.md 8(d).  `only`: one op's name
    (the profiler passes of tools/summarize/per_op_budget.py run one op per process)"""
    L = ll.lib()
    ctx = ll.Context(15, 14)
    N, K = ctx.N, ctx.K
    a, b, d = ll.DeviceBuffer((2, ell, N)), ll.DeviceBuffer((2, ell, N)), ll.DeviceBuffer((2, ell, N))
    key = ll.DeviceBuffer((K - 1, 2, K, N))
    for buf, v in ((a, 1), (b, 2), (key, 3)):
        L.dc_memset(buf.ptr, v, buf.nbytes)
    st = ell * N
    e0, e1 = L.dc_event_create(), L.dc_event_create()
    p_limb = 8 * N
    ops = {
        "rotate_hop": (lambda: L.dc_ct_rotate_hop(ctx.h, d.ptr, st, a.ptr, st, 3, key.ptr, ell, None), (2 * ell * ell + 7 * ell) * p_limb, 150699),
        "mulcc_relin": (lambda: L.dc_ct_mul_relin(ctx.h, d.ptr, st, a.ptr, st, b.ptr, st, key.ptr, ell, None),
                        (4 * ell + 2 * ell * ell + 7 * ell) * p_limb, 160732),
        "rescale": (lambda: L.dc_ct_rescale(ctx.h, d.ptr, st, a.ptr, st, ell, None), (2 * ell + 2 * (ell - 1)) * p_limb, 17418),
    }
    out = {}
    for name, (fn, nbytes, ref_us) in ops.items():
        if only and name != only:
            continue
        fn()
        L.dc_event_record(e0, None)
        for _ in range(iters):
            fn()
        L.dc_event_record(e1, None)
        us = L.dc_event_elapsed_ms(e0, e1) / iters * 1e3
        out[name] = {"us": round(us, 1), "algorithmic_bytes": nbytes, "achieved_gbs": round(nbytes / (us * 1e-6) / 1e9, 1),
                     "frac_of_hbm_peak": round(nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4), "reference_seal_cpu_us": ref_us}
    out["level"] = ell
    out["reference_table"] = "profiled_SEAL_CPU.json:10-45 (hardware unstated)"
    return out


def ntt_micro_leg(ll, iters=200):
    """BASELINE config 2: single forward NTT, N = 2^14, 1 limb (latency-bound)"""
    L = ll.lib()
    ctx = ll.Context(14, 2)
    buf = ll.DeviceBuffer((1, ctx.N))
    L.dc_memset(buf.ptr, 1, buf.nbytes)
    for _ in range(5):
        ctx.ntt(buf, 1)
    e0, e1 = L.dc_event_create(), L.dc_event_create()
    L.dc_event_record(e0, None)
    for _ in range(iters):
        ctx.ntt(buf, 1)
    L.dc_event_record(e1, None)
    us = L.dc_event_elapsed_ms(e0, e1) / iters * 1e3
    return {"workload": "single forward NTT, N=2^14, 1 limb", "us_per_ntt_back_to_back": round(us, 2)}


def cfg3_leg(ll, iters=5, grouped=True):
    """BASELINE config 3: one ct x ct multiply + relinearise at N = 2^16, 24 data primes + 1 special (bit-exactness of this
    size is tests/test_gpu_ops.py::test_baseline_config3_...).  Operands are constant-filled canonical residues: timing only.
    Algorithmic bytes per SURVEY.md 8(d): (4l [in] + l [target] + 2l(l+1) [key] + 4l [ct RMW]) * P_limb = 708 MiB."""
    L = ll.lib()
    logN, K = 16, 25
    ctx = ll.Context(logN, K)
    N, ell = 1 << logN, K - 1
    a, b, d = ll.DeviceBuffer((2, ell, N)), ll.DeviceBuffer((2, ell, N)), ll.DeviceBuffer((2, ell, N))
    key = ll.DeviceBuffer((K - 1, 2, K, N))
    for buf, v in ((a, 1), (b, 2), (key, 3)):
        L.dc_memset(buf.ptr, v, buf.nbytes)
    st = ell * N
    L.dc_ct_mul_relin(ctx.h, d.ptr, st, a.ptr, st, b.ptr, st, key.ptr, ell, None)
    e0, e1 = L.dc_event_create(), L.dc_event_create()
    L.dc_event_record(e0, None)
    for _ in range(iters):
        L.dc_ct_mul_relin(ctx.h, d.ptr, st, a.ptr, st, b.ptr, st, key.ptr, ell, None)
    L.dc_event_record(e1, None)
    us = L.dc_event_elapsed_ms(e0, e1) / iters * 1e3
    alg = (4 * ell + ell + 2 * ell * (ell + 1) + 4 * ell) * N * 8
    ntts = (ell + 1) * (ell + 2)
    out = {"workload": "ct x ct multiply + relinearise, N=2^16, 24+1 primes, 1 ciphertext pair", "us": round(us, 1),
           "ntt_equivalents": ntts, "ntt_per_s": round(ntts / (us * 1e-6)), "algorithmic_bytes": alg,
           "achieved_gbs": round(alg / (us * 1e-6) / 1e9, 1), "frac_of_hbm_peak": round(alg / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
    del ctx, key
    if not grouped:  # (the profiler passes of tools/summarize/per_op_budget.py: SEAL-mode launches only)
        return out
    # the same product under grouped-digit keys (EXTENSION, hybrid_ks.hip: not SEAL's scheme): 24 data primes in 3 digits of 8, 8 special primes
    ks = alpha = 8
    ctx2 = ll.Context(logN, ell + ks, special=ks, alpha=alpha)
    G, M = -(-ell // alpha), ell + ks
    key2 = ll.DeviceBuffer((ctx2.key_digits, 2, ell + ks, N))
    L.dc_memset(key2.ptr, 3, key2.nbytes)
    L.dc_ct_mul_relin(ctx2.h, d.ptr, st, a.ptr, st, b.ptr, st, key2.ptr, ell, None)
    L.dc_event_record(e0, None)
    for _ in range(iters):
        L.dc_ct_mul_relin(ctx2.h, d.ptr, st, a.ptr, st, b.ptr, st, key2.ptr, ell, None)
    L.dc_event_record(e1, None)
    us2 = L.dc_event_elapsed_ms(e0, e1) / iters * 1e3
    E = G * M - ell
    alg2 = (4 * ell + 4 * ell + (2 * ell + 2 * G * M + 2 * ell) + (ell + E) + (E + ell + 2 * G * M + 2 * M) + (2 * ks + 2 * ell) + 6 * ell) * N * 8
    ntts2 = G * M + 2 * ks + 2 * ell
    out["grouped_digit_keys"] = {"workload": f"the same product with {G} digits of {alpha} primes and {ks} special primes (extension; key {key2.nbytes >> 20} MiB "
                                             f"instead of {(ell * 2 * (ell + 1) * N * 8) >> 20} MiB)", "us": round(us2, 1), "ntt_equivalents": ntts2,
                                 "algorithmic_bytes": alg2, "achieved_gbs": round(alg2 / (us2 * 1e-6) / 1e9, 1),
                                 "frac_of_hbm_peak": round(alg2 / (us2 * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
    return out


def _cpu_prefix(o, cst: bytes, hv: bytes, image, budget_s: float, threads: int):
    """the oracle VM on a prefix of a program for `budget_s` seconds of run-time ops: (NTT-equivalents, seconds, ops, key switches)"""
    import tempfile

    from oracle.oracle import OracleVM

    o.L.orc_set_threads(threads)
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "p.cst").write_bytes(cst)
        (Path(d) / "p.hevm").write_bytes(hv)
        vm = OracleVM(o)
        vm.load(Path(d) / "p.cst", Path(d) / "p.hevm")
    vm.encrypt(0, image)
    ntts, n_ops, spent, ks = 0, 0, 0.0, 0
    for op in vm.prog.ops:
        opcode, dst, lhs, rhs = (int(x) for x in op)
        if opcode == 0:  # encode lazily, untimed (preprocess is untimed in the reference)
            src = np.ones(1) if lhs == 0xFFFF else vm.consts[lhs]
            vm.plains[dst] = vm.encode_internal(src, rhs >> 10, rhs & 0x3FF)
            continue
        lvl = vm.ciphers[lhs].ell
        t = time.perf_counter()
        vm.step(op)
        spent += time.perf_counter() - t
        n_ops += 1
        if opcode == 1:
            off = rhs - 65536 if rhs >= 32768 else rhs
            h = len(o.rotate_hops(off))
            ntts += h * (lvl + 1) * (lvl + 2)
            ks += h
        elif opcode == 8:
            ntts += (lvl + 1) * (lvl + 2)
            ks += 1
        elif opcode == 3:
            ntts += 2 * lvl
        if spent > budget_s:
            break
    o.L.orc_set_threads(1)
    return ntts, spent, n_ops, ks


def cpu_baseline_leg(cst: bytes, hv: bytes, image, budget_s=15.0, hv_b13: bytes | None = None, openmp=True):
    """The CPU path timed beside the GPU: the oracle VM (oracle/: a restatement of SEAL's algorithms, the reference's arithmetic being
    unbuildable here) on a PREFIX of the same program.  `value` = 1 thread, like SEAL's evaluator and the reference's HEVM loop; beside it
    the 8-thread OpenMP-over-limbs variant BASELINE.md names, and both again on the b13 lowering (key switches at up to 13 primes: the
    plan shape the reference's own SEAL cost table implies, profiled_SEAL_CPU.json:5-8), where limb parallelism has something to chew on."""
    import os as _os

    from oracle.oracle import Oracle

    t0 = time.time()
    o = Oracle(15, 14)
    o.keygen(seed=0x4845564D)
    setup_s = time.time() - t0
    ncpu = _os.cpu_count() or 1
    th = min(8, ncpu)
    ntts, spent, n_ops, ks = _cpu_prefix(o, cst, hv, image, budget_s, 1)
    out = {"value": round(ntts / spent, 1), "unit": "NTT/s", "cores": 1, "kind": "port",
           "sample": f"first {n_ops} run-time ops ({ks} key switches) of the same HEVM program, "
                     f"{spent:.1f} s of single-thread work (+{setup_s:.0f} s untimed keygen)",
           "seconds": round(spent, 2), "ntt_equivalents": ntts, "host_cpus": ncpu,
           "reference_published": "README.md:176-188: 53.73 s for the DaCapo-compiled ResNet-20 on SEAL CPU (hardware unstated)"}
    if openmp and o.L.orc_has_openmp() and th > 1:
        _cpu_prefix(o, cst, hv, image, 0.5, th)  # thread-pool warm-up
        n2, s2, ops2, ks2 = _cpu_prefix(o, cst, hv, image, budget_s / 2, th)
        out["openmp"] = {"value": round(n2 / s2, 1), "unit": "NTT/s", "cores": th,
                         "sample": f"first {ops2} run-time ops ({ks2} key switches), {s2:.1f} s, OpenMP over the limbs of each op",
                         "note": "at 1-3 primes an op has 2-4 limbs to spread: little to gain on the headline lowering"}
    if hv_b13 is not None:
        n3, s3, ops3, ks3 = _cpu_prefix(o, cst, hv_b13, image, budget_s / 2, 1)
        out["b13_lowering"] = {"value": round(n3 / s3, 1), "unit": "NTT/s", "cores": 1,
                               "sample": f"first {ops3} run-time ops ({ks3} key switches at up to 13 primes) of tests/golden/resnet20.b13, {s3:.1f} s"}
        if o.L.orc_has_openmp() and th > 1:
            n4, s4, ops4, ks4 = _cpu_prefix(o, cst, hv_b13, image, budget_s / 2, th)
            out["b13_lowering"]["openmp"] = {"value": round(n4 / s4, 1), "unit": "NTT/s", "cores": th,
                                             "sample": f"first {ops4} run-time ops ({ks4} key switches), {s4:.1f} s"}
    return out


def ks_traffic_record(per_op, cfg3):
    """measured HBM bytes (FETCH_SIZE x 2 + WRITE_SIZE, summed over an op's launches) over SURVEY 8(d)'s algorithmic bytes, for the rotation hop
    at 13 primes and config 3: from profiles/<round>_per_op_budget_<op>.json (tools/collect_per_op_budget.sh), reported only when those passes ran
    on exactly the library being timed"""
    out = {}
    for name, op, alg in (("hop13", "rotate_hop", per_op.get("rotate_hop", {}).get("algorithmic_bytes")), ("cfg3", "cfg3", cfg3.get("algorithmic_bytes"))):
        f = ROOT / "profiles" / f"{PROF}_per_op_budget_{op}.json"
        if not f.exists() or not alg:
            continue
        rec = json.loads(f.read_text())
        if rec.get("lib_sha256") != lib_sha256():
            continue
        moved = sum((k["read_MB"] + k["write_MB"]) * 1e6 * k.get("launches_per_op", 1) for k in rec["kernels"])
        out[name] = {"hbm_bytes": moved, "algorithmic_bytes": alg, "traffic_over_algorithmic": round(moved / alg, 3),
                     "source": f"profiles/{PROF}_per_op_budget_{op}.json"}
    return out or None


LINE_LIMIT = 4096  # bytes of the final stdout line: the driver's parser reads the tail of stdout (round 5's 22.5 KB line did not parse)


def compact_line(full: dict) -> dict:
    """The ONE line the driver parses: the contract's fields + roofline + cpu_baseline + a handful of scalars; numbers and short names only.
    Everything else (legs, tables, prose) is the full record (--out).  tests/test_bench_line.py holds it to LINE_LIMIT on a full-size stub."""
    g = lambda d, *ks: (g(d.get(ks[0]), *ks[1:]) if len(ks) > 1 else d.get(ks[0])) if isinstance(d, dict) else None
    cfg = full.get("config") or {}
    line = {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                                    "dtype", "data")}
    line["config"] = {"workload": str(cfg.get("workload", ""))[:300], "key_switches_per_step": cfg.get("key_switches_per_step"),
                      "ntt_equivalents_per_step": cfg.get("ntt_equivalents_per_step"), "streams_per_gpu": cfg.get("streams_per_gpu"),
                      "parallelism": cfg.get("parallelism")}
    r = full.get("roofline")
    if r:
        dom = g(r, "step", "dominant") or {}
        moved, alg = g(r, "step", "bytes_actually_moved"), g(r, "step", "algorithmic_bytes")
        line["roofline"] = {"bound": r.get("bound"), "achieved": r.get("achieved"), "peak": r.get("peak"), "unit": r.get("unit"), "frac": r.get("frac"),
                            "traffic": r.get("traffic"), "kernel": str(r.get("kernel", "")).split(" ")[0], "avg_us": g(r, "launch", "avg_us"),
                            "algorithmic_bytes": g(r, "launch", "algorithmic_bytes"),
                            "step_frac": g(r, "step", "frac"), "step_achieved": g(r, "step", "achieved_gbs"),
                            "step_traffic_over_algorithmic": (round(moved / alg, 3) if moved and alg else None),
                            "dominant_kernel": (str(dom.get("kernel"))[:80] if dom else None), "dominant_frac": dom.get("hbm_frac_of_peak")}
    c = full.get("cpu_baseline")
    if c:
        line["cpu_baseline"] = {k: c.get(k) for k in ("value", "unit", "cores", "kind", "sample", "seconds")}
        line["cpu_baseline"]["sample"] = str(c.get("sample", ""))[:200]
        line["speedup_vs_cpu_port"] = full.get("speedup_vs_cpu_port")
    line["rms_vs_torch"] = g(full, "decrypted_error", "rms_vs_torch")
    c4 = full.get("config4_resnet20_nt65536_N131072")
    if c4:
        line["config4"] = ({"error": str(c4["error"])[:120]} if "error" in c4 else
                           {"run_s": c4.get("run_s"), "rms_vs_torch": c4.get("rms_vs_torch"), "bootstraps": c4.get("real_bootstraps"),
                            "bootstraps_reference_plan": c4.get("bootstraps_reference_plan"), "key_switches": c4.get("key_switches"),
                            "lazy_sums_run_s": g(c4, "lazy_sums", "run_s"), "lazy_sums_rms_vs_torch": g(c4, "lazy_sums", "rms_vs_torch"),
                            "double_hoist_run_s": g(c4, "lazy_sums_double_hoist", "run_s"),
                            "double_hoist_rms_vs_torch": g(c4, "lazy_sums_double_hoist", "rms_vs_torch")})
    line["cfg3_us"], line["cfg3_frac"] = g(full, "cfg3_mul_relin", "us"), g(full, "cfg3_mul_relin", "frac_of_hbm_peak")
    po = full.get("per_op_13_primes") or {}
    line["per_op_13_us"] = {k: g(po, k, "us") for k in ("rotate_hop", "mulcc_relin", "rescale") if k in po} or None
    kt = full.get("ks_traffic") or {}
    line["ks_traffic_over_algorithmic"] = {k: v.get("traffic_over_algorithmic") for k, v in kt.items()} or None
    line["ntt_micro_us"] = g(full, "ntt_micro", "us_per_ntt_back_to_back")
    line["full_record"] = full.get("full_record")
    # belt and braces: should a field ever grow, drop the optional ones (last first) rather than emit a line the driver cannot parse
    for k in ("full_record", "ntt_micro_us", "ks_traffic_over_algorithmic", "per_op_13_us", "cfg3_frac", "cfg3_us", "config4", "rms_vs_torch"):
        if len(json.dumps(line)) <= LINE_LIMIT:
            break
        line.pop(k, None)
    return line


def emit(full: dict, out=None):
    """write the full record to `out` (default gpurun_out/bench_full.json: merged back by gpurun, git-ignored), then print the compact line as the
    LAST line of stdout"""
    path = Path(out) if out else ROOT / "gpurun_out" / "bench_full.json"
    try:
        path.parent.mkdir(parents=True, exist_ok=True)
        full["full_record"] = str(path.relative_to(ROOT)) if path.is_relative_to(ROOT) else str(path)
        path.write_text(json.dumps(full, indent=1))
    except OSError as e:  # a read-only tree must not cost the line
        full["full_record"] = None
        print(f"[bench] full record not written: {e}", file=sys.stderr)
    text = json.dumps(compact_line(full))
    assert len(text) <= LINE_LIMIT, len(text)
    sys.stdout.flush()
    print(text, flush=True)
    return path


DUMP_LIMIT = 64 << 20  # bytes, all files of one --dump-outputs together


def read_outputs(hevm, streams: int) -> list:
    """getOutput() of every stream (decrypted, decoded: what the reference's runner hands its caller), stream 0 selected afterwards"""
    outs = []
    for s in range(streams):
        hevm.select_stream(s)
        outs.append(hevm.getOutput())
    hevm.select_stream(0)
    return outs


def dump_outputs(d, outs: list):
    """--dump-outputs: outs[s] -> d/output.npy (s = 0) and d/output_stream<s>.npy, float64"""
    arrays = {("output" if s == 0 else f"output_stream{s}"): np.ascontiguousarray(o, dtype=np.float64) for s, o in enumerate(outs)}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT:
        raise SystemExit(f"[bench] --dump-outputs: {total} bytes of outputs exceed {DUMP_LIMIT}")
    path = Path(d)
    path.mkdir(parents=True, exist_ok=True)
    for name, a in arrays.items():
        np.save(path / f"{name}.npy", a)
    print(f"[bench] outputs: {', '.join(f'{n}.npy {a.shape}' for n, a in arrays.items())} in {path}", file=sys.stderr)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--program", default="resnet20", choices=["resnet20", "shaped", "config4"],
                    help="resnet20 = the reference model's traced op stream + real weights (tests/golden); shaped = synthetic op mix; "
                         "config4 = BASELINE config 4's stream (nt = 2^16 trace, N = 2^17, real bootstraps, grouped-digit keys) as the timed "
                         "step: with --gpus N this is BASELINE config 5, one such stream per GPU")
    ap.add_argument("--hevm-gz", default=None, help="--program resnet20: another lowering of the same trace (same constants)")
    ap.add_argument("--layers", type=int, default=20, help="--program shaped: depth (20 = the traced op mix)")
    ap.add_argument("--streams", type=int, default=1, help="independent ciphertext streams per GPU (throughput mode; 1 = the reference's one image per run)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline: the decrypted error vs the torch model, the roofline leg, the NTT micro leg, "
                         "config 3, the per-op leg, the CPU baseline, config 4 in a child process, and the A/B legs that only the full record "
                         "carries: the b6 / b13 lowerings, direct rotation keys, the streams table, real bootstrapping at N = 2^15, config 3 under "
                         "grouped-digit keys, config 4's key shapes / chains / key sets, the CPU baseline with OpenMP and on the b13 lowering "
                         "(several minutes more).  Without it the run measures the headline only")
    ap.add_argument("--out", default=None,
                    help="where the FULL record goes (with --full, a default side file when not given; a plain run writes one only when "
                         "given); stdout's last line is the compact line (<= 4 KB)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one computed -- the decrypted result, getOutput() of every stream -- as "
                         "DIR/output.npy (stream 0) and DIR/output_stream<s>.npy (float64).  The inputs are the same from run to run; keys and "
                         "encryption randomness come from the OS, so two runs agree to within CKKS noise (~1e-7 rms), not bit for bit")
    ap.add_argument("--no-lowerings", action="store_true", help="--full: skip the other lowerings of the trace (config.lowerings)")
    ap.add_argument("--no-streams-leg", action="store_true", help="--full: skip the throughput table (1 / 2 / 4 / 8 / 16 streams of the headline program in one VM)")
    ap.add_argument("--config4-lazy-sums", type=int, default=0,
                    help="--program config4: VM option hyb_lazy_sum for the timed stream (0 = the library's default: every rotate instruction "
                         "rounds on its own, the reference's semantics; 1 = one division by P per sum of rotations)")
    ap.add_argument("--no-config4", dest="config4", action="store_false",
                    help="--full: skip BASELINE config 4's shape (ResNet-20 traced at nt = 2^16, N = 2^17, real bootstrapping; ~1 min, ~180 GB of "
                         "HBM); with --full it runs by default, in a child process before this one touches the GPU")
    ap.add_argument("--config4", dest="config4", action="store_true", help="(default with --full)")
    ap.set_defaults(config4=True)
    ap.add_argument("--broadcast-keys", action="store_true",
                    help="every rank generates its own key set, then rank 0's is shipped to the others (one flat RCCL broadcast per key "
                         "buffer) and the ranks compare key digests: the default with more than one rank (the flag forces the path at world size 1)")
    ap.add_argument("--dry-run", action="store_true",
                    help="exercise the launch / rank / aggregation path without a GPU: no kernel runs, the step is a sleep, the process "
                         "group uses gloo (tests/test_dist_gloo.py)")
    return ap


def _config4_run(args):
    import subprocess

    cmd = [sys.executable, str(ROOT / "tools" / "legs" / "resnet_real_boot.py")] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True)
    last = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not last:
        return {"error": f"tools/legs/resnet_real_boot.py exited with {r.returncode}", "stderr_tail": r.stderr[-400:]}
    res = json.loads(last[-1])
    res["command"] = "python tools/legs/resnet_real_boot.py " + " ".join(str(a) for a in args)
    return res


def config4_child(full=False):
    """BASELINE config 4's shape -- ResNet-20 traced at the reference script's own nt = 2^16 slots (examples/benchmarks/ResNet.py:50), run
    on N = 2^17 (HEAAN_HEVM.cpp:55-56) with a real bootstrap at every bootstrap site (tools/legs/resnet_real_boot.py).  About 180 GB of keys
    and plaintexts: it runs in a CHILD process started before this one touches the GPU.  One child, two VMs one after the other: the
    library's default options first (`run_s`: every rotate instruction rounds on its own, the reference's semantics), then the same lowered
    program with VM option hyb_lazy_sum = 1 (`lazy_sums.run_s`: one division by P per sum of rotations -- other limbs, replayed by the
    oracle VM in tests/test_gpu_config4_geometry.py -- a labelled extension, never the like-for-like figure).  --full adds rounds 3-5's
    A/B children (key shapes, chains, bounded key sets)."""
    ks, al = CONFIG4["ks_special"], CONFIG4["ks_alpha"]
    res = _config4_run([1, CONFIG4["fixture"], CONFIG4["logN"], CONFIG4["msg_bits"], CONFIG4["lowering"], ks, al, "--also-opt", "hyb_lazy_sum=1",
                        "--also-opt", "hyb_lazy_sum=1,hyb_double_hoist=1"])
    if "error" in res:
        return res
    also = res.pop("also", None) or [None, None]
    lazy, dh = also[0], (also[1] if len(also) > 1 else None)
    res["program"] = ("tests/golden/resnet20_nt16.b14: bootstraps at the model script's own hints (before every activation), each restoring 14 "
                      "primes -> 38 real bootstraps; 31 data + 9 special 60-bit primes")
    res["bootstraps_reference_plan"] = 19  # README.md:131-136: DaCapo's own plan for HEaaN places 19 (placement is the compiler's, out of scope)
    res["keys"] = ("grouped-digit hybrid key switching (extension, hybrid_ks.hip / hybrid_fused.hip): 4 digits of 8 primes, P = 9 primes; one "
                   "direct Galois key per rotation offset (286 keys x 0.34 GB)")
    res["security"] = "N = 2^17, log2(QP) = 40 x 60 = 2400 bits, sparse ternary secret (h = 64): inside the 128-bit range for N = 2^17"
    res["reference"] = "README.md:131-136: DaCapo's cost model estimates 13.6 s for its 19-bootstrap HEaaN plan (not measured)"
    brief = lambda r: ({k: r.get(k) for k in ("chain", "log2_QP", "primes", "special_primes", "primes_per_digit", "rotation_keys", "rotation_key_bytes",
                                             "rot_compose", "run_s", "key_switches", "ntt_equivalents", "rms_vs_torch", "fixture", "command", "lazy_sums")}
                       if "error" not in r else r)
    res["lazy_sums"] = brief(lazy) if lazy else None  # (the extension's figure, beside -- not instead of -- run_s)
    res["lazy_sums_double_hoist"] = brief(dh) if dh else None  # (option hyb_double_hoist on top: taps times a plaintext join the sums)
    if not full:
        return res
    lz = ["--opt", "hyb_lazy_sum=1"]
    res["key_shapes"] = {"digits_of_8_under_9": brief(res), "digits_of_7_under_8": brief(_config4_run([1, "resnet20_nt16", 17, 1, "b14", 8, 7]))}
    res["chains"] = {"chain_60": brief(res), "chain_mixed": brief(_config4_run([1, "resnet20_nt16", 17, 1, "b14r51", ks, al, "mixed_app"]))}
    res["key_sets"] = {"49": brief(_config4_run([49, "resnet20_nt16", 17, 1, "b14", ks, al])),
                       "96": brief(_config4_run([96, "resnet20_nt16", 17, 1, "b14", ks, al])),
                       "286": brief(res),
                       "96_lazy_sums": brief(_config4_run([96, "resnet20_nt16", 17, 1, "b14", ks, al] + lz))}
    return res


# digits of 8 primes under 9 special primes (round 5: 4 digits at the top level, 96 GB of rotation keys).  lazy_sums = VM option hyb_lazy_sum of
# `--program config4` (BASELINE config 5's stream): the library's default, 0, unless --config4-lazy-sums asks for the extension
CONFIG4 = {"fixture": "resnet20_nt16", "lowering": "b14", "logN": 17, "ks_special": 9, "ks_alpha": 8, "msg_bits": 1, "secret_hw": 64, "lazy_sums": 0}


def config4_program():
    """BASELINE config 4's program: the nt = 2^16 trace whose 38 bootstrap sites (the model script's own hints, each restoring 14 primes) are
    lowered to real CKKS bootstrapping (dacapo_amd/ckks_boot.py).  Returns (fixture, constants, bytecode, primes in the chain, rotation offsets)."""
    import gzip

    from dacapo_amd import ckks_boot as cb
    from dacapo_amd import hevm_asm as ha

    g = ROOT / "tests" / "golden"
    fx = ha.read_fixture(g / CONFIG4["fixture"])
    hv0 = gzip.open(g / f"{CONFIG4['fixture']}.{CONFIG4['lowering']}.hevm.gz").read()
    target = {int(r) for o, _, _, r in ha.unpack_hevm(hv0)["ops"].tolist() if o == ha.OP_BOOTSTRAP}
    assert len(target) == 1
    K = target.pop() + cb.boot_levels() + CONFIG4["ks_special"]
    hv, cst = cb.lower_bootstraps(hv0, fx["cst"], CONFIG4["logN"], K, msg_bits=CONFIG4["msg_bits"], ks=CONFIG4["ks_special"])
    return fx, cst, hv, K, cb.rotation_offsets(hv)


def config4_ntt_equivalents(hv, K):
    """NTT-equivalents of one run of the program, counted per key switch as the grouped-digit sequence executes it without sharing:
    G (l + k) + 2 k + 2 l per hop, 2 l per rescale (what hevm_last_run_stats reports on the device)"""
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import progstats

    st = progstats.walk(hv, CONFIG4["logN"], direct_keys=True)
    k, a = CONFIG4["ks_special"], CONFIG4["ks_alpha"]
    ks = sum(n * (-(-int(l) // a) * (int(l) + k) + 2 * k + 2 * int(l)) for l, n in st["key_switch_level_histogram"].items())
    rs = sum(n * 2 * int(l) for l, n in st.get("rescale_level_histogram", {}).items())
    return int(ks + rs), st


def main_config4(args, grp):
    """--program config4 [--gpus N]: every rank runs BASELINE config 4's stream on its own GPU -- own VM, the SAME key set (same seed, or
    --broadcast-keys; digests compared), its own input -- no collective in the op path: with N = 8 this is BASELINE config 5.  The timed step
    is one run() (38 real bootstraps, ~10 k key switches, seconds): keep --steps small."""
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    rank, local_rank, world = grp.rank, grp.local_rank, grp.world
    CONFIG4["lazy_sums"] = int(args.config4_lazy_sums)
    fx, cst, hv, K, offs = config4_program()
    L = ll.lib()
    L.dc_set_device(local_rank)

    def barrier_sync():
        grp.barrier()
        L.dc_device_sync()

    t_setup = time.time()
    hevm = runner.HEVM(fresh=True, logN=CONFIG4["logN"], num_primes=K, ks_special=CONFIG4["ks_special"],
                       ks_alpha=CONFIG4["ks_alpha"], vm_options={"secret_hw": CONFIG4["secret_hw"], "hyb_lazy_sum": CONFIG4["lazy_sums"]})
    hevm.addRotationKeys(offs)  # (before the digest: the direct keys are part of the replicated key set)

    def _copy_out(ptr, words):
        import torch

        t = torch.empty(words, dtype=torch.int64, device=grp.device)
        L.dc_memcpy_d2d(t.data_ptr(), ptr, 8 * words, None)
        L.dc_device_sync()
        return t

    def _copy_in(ptr, t):
        import torch

        torch.cuda.synchronize()
        L.dc_memcpy_d2d(ptr, t.data_ptr(), 8 * t.numel(), None)
        L.dc_device_sync()

    share = args.broadcast_keys or world > 1  # every rank generated its own set; rank 0's is shipped to the others (RCCL broadcasts out of HBM)
    key_info = grp.share_keys(hevm.keyDigest, buffers_fn=hevm.keyBuffers, copy_out=_copy_out, copy_in=_copy_in, mode="broadcast" if share else "local")
    if share and rank != 0:
        hevm.keysReplaced()
    image = fx["packed"] if rank == 0 else np.roll(fx["packed"], 17 * rank) * (1.0 - 0.01 * rank)
    hevm.load_mem(cst, hv)
    hevm.setInput(0, image)
    t_setup = time.time() - t_setup
    for _ in range(args.warmup):
        hevm.run()
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        hevm.run()
    barrier_sync()
    elapsed = time.perf_counter() - t0
    stats = hevm.stats()
    outs = read_outputs(hevm, 1)
    out = outs[0][0]
    elapsed, total = grp.job_totals(elapsed, float(stats["ntts"]) * args.steps)
    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, outs)
        rms = float(np.sqrt(np.mean((out[:10] * 32 - fx["torch_result"]) ** 2)))
        print(json.dumps(config4_line(args, world, elapsed, total, stats["ntts"], stats["keyswitches"], key_info, t_setup, rms, len(offs), K)), flush=True)
    hevm.close()
    grp.close()


def config4_line(args, world, elapsed, total, ntts_per_step, ks_per_step, key_info, t_setup, rms, n_keys, K, dry=False):
    N = 1 << CONFIG4["logN"]
    key_bytes = n_keys * (-(-(K - CONFIG4["ks_special"]) // CONFIG4["ks_alpha"])) * 2 * K * N * 8
    return {"metric": "NTT/s (NTT-equivalents of N = 2^17 over one run() of the ResNet HEVM program traced at nt = 2^16: BASELINE config 4's stream"
                      + (", dry run: no kernel executed)" if dry else ")"),
            "value": round(total / elapsed, 1), "unit": "NTT/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u64",
            "data": "none (dry run)" if dry else "synthetic image; weights = the reference's resnet20.silu.model", "dry_run": dry,
            "measured_on_hardware": not dry,
            "config": {"workload": f"BASELINE config {5 if world > 1 else 4}: ResNet-20 (SiLU) traced at nt = 2^16 slots, N = 2^17, {K} x 60-bit primes "
                                   f"({K - CONFIG4['ks_special']} data + {CONFIG4['ks_special']} special), 38 real bootstraps each restoring 14 primes, "
                                   "grouped-digit hybrid key switching" + (", lazy sums (option hyb_lazy_sum)" if CONFIG4["lazy_sums"] else "")
                                   + ", one independent ciphertext stream per GPU",
                       "ntt_equivalents_per_step": ntts_per_step, "key_switches_per_step": ks_per_step, "rotation_keys": n_keys,
                       "key_bytes_per_gpu": key_bytes, "streams_per_gpu": 1,
                       "parallelism": f"replicas x{world} (no collective in the op path)", "keys": key_info},
            "hevm_wall_s": round(elapsed / args.steps, 3), "setup_s_untimed": round(t_setup, 1),
            "decrypted_error": None if rms is None else {"rms_vs_torch": rms, "reference_published_rms": 9.5e-4}}


def spawn_ranks(args, argv) -> int:
    """`python bench.py --gpus N` outside a launcher: start N ranks as a CHILD torch.distributed.run (this parent has not touched the
    GPU and never does -- a process that has initialised HIP must not exec another program on this pool) and hand its exit code back."""
    import socket
    import subprocess

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", port, str(Path(__file__).resolve())] + list(argv)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this pool (RCCL needs it)
    return subprocess.call(cmd, env=env)


def dry_run(args, grp):
    """The rank / barrier / aggregation / JSON path of a real run with the device work replaced by a sleep."""
    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import progstats

    cfg4 = args.program == "config4"
    if cfg4:  # config 5's launch path: the same lowering and work count as the real run, the device work replaced by a sleep
        _, _, hv4, K4, offs4 = config4_program()
        ntts4, st4 = config4_ntt_equivalents(hv4, K4)
        st = {"ntt_equivalents": ntts4}
    else:
        fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
        st = progstats.walk(fx["hevm"])
    # the key-replication path with stand-in buffers (three "keys" of 4096 words expanded from the seed): same code as the real run's
    import hashlib

    import torch

    share = args.broadcast_keys or grp.world > 1  # as in the real run: per-rank sets, rank 0's broadcast whenever there is more than one rank
    seed = KEY_SEED + (grp.rank if share else 0)
    fake = [torch.from_numpy(np.random.default_rng([seed, i]).integers(0, 1 << 62, 4096, dtype=np.int64)) for i in range(3)]
    keys = grp.share_keys(lambda: int.from_bytes(hashlib.sha256(b"".join(t.numpy().tobytes() for t in fake)).digest()[:8], "little"),
                          buffers_fn=lambda: [(i, 4096) for i in range(3)], copy_out=lambda i, w: fake[i].clone(),
                          copy_in=lambda i, t: fake[i].copy_(t), mode="broadcast" if share else "local")
    for _ in range(args.warmup):
        time.sleep(0.001)
    grp.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.002)
    grp.barrier()
    elapsed = time.perf_counter() - t0
    elapsed, total = grp.job_totals(elapsed, float(st["ntt_equivalents"]) * args.steps)
    if grp.rank == 0 and cfg4:
        print(json.dumps(config4_line(args, grp.world, elapsed, total, st["ntt_equivalents"], int(sum(st4["key_switch_level_histogram"].values())), keys, 0.0,
                                      None, len(offs4), K4, dry=True)), flush=True)
    elif grp.rank == 0:
        print(json.dumps({"metric": "NTT/s (dry run: no kernel executed)", "value": round(total / elapsed, 1), "unit": "NTT/s",
                          "n_gpus": grp.world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u64", "data": "none (dry run)",
                          "dry_run": True, "keys": keys,
                          "config": {"workload": "dry run", "ntt_equivalents_per_step": st["ntt_equivalents"], "streams_per_gpu": args.streams,
                                     "parallelism": f"replicas x{grp.world} (no collective in the op path)"}}), flush=True)
    grp.close()


def main():
    argv = sys.argv[1:]
    args = build_parser().parse_args(argv)
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(args, argv))

    # --full, rank 0 of a 1-GPU run only: the other legs of the line are N = 1 figures as well
    config4 = config4_child(args.full) if (args.full and args.config4 and args.gpus == 1 and not args.dry_run and "RANK" not in os.environ
                                           and args.program != "config4") else None

    from dacapo_amd.dist import Group

    grp = Group(backend="gloo" if args.dry_run else "nccl")
    rank, local_rank, world = grp.rank, grp.local_rank, grp.world
    if world != args.gpus and rank == 0:
        print(f"[bench] --gpus {args.gpus} but the launcher started {world} rank(s): reporting n_gpus = {world}", file=sys.stderr)
    if args.dry_run:
        return dry_run(args, grp)
    if args.program == "config4":
        return main_config4(args, grp)

    from dacapo_amd import hevm_asm as ha
    from dacapo_amd import lowlevel as ll
    from dacapo_amd import runner

    L = ll.lib()
    L.dc_set_device(local_rank)

    def barrier_sync():
        grp.barrier()  # dist.barrier() + torch.cuda.synchronize() when world > 1
        L.dc_device_sync()

    # ---- set-up (untimed, like hc-test: context/keys, load, preprocess, encrypt) ---------------------------------
    t_setup = time.time()
    # replicas serve ONE client: every rank holds the same key set.  Every rank generates a set on its own GPU, then rank 0's
    # is broadcast (one flat RCCL broadcast per key buffer) and the ranks compare device-side digests.  Inputs and encryption randomness differ per rank.
    hevm = runner.HEVM(fresh=True, logN=15, num_primes=14)  # (hevm_init_fresh: keys from the OS's randomness -- the release build has no seeded keygen)
    if args.streams > 1:
        hevm.set_streams(args.streams)

    def _copy_out(ptr, words):
        import torch

        t = torch.empty(words, dtype=torch.int64, device=grp.device)
        L.dc_memcpy_d2d(t.data_ptr(), ptr, 8 * words, None)
        L.dc_device_sync()
        return t

    def _copy_in(ptr, t):
        import torch

        torch.cuda.synchronize()
        L.dc_memcpy_d2d(ptr, t.data_ptr(), 8 * t.numel(), None)
        L.dc_device_sync()

    share = args.broadcast_keys or world > 1  # every rank generated its own set; rank 0's is shipped to the others (RCCL broadcasts out of HBM)
    key_info = grp.share_keys(hevm.keyDigest, buffers_fn=hevm.keyBuffers, copy_out=_copy_out, copy_in=_copy_in, mode="broadcast" if share else "local")
    if share and rank != 0:
        hevm.keysReplaced()
    fx = None
    if args.program == "resnet20":
        fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
        cst, hv, info = fx["cst"], fx["hevm"], fx["meta"]["info"]
        if args.hevm_gz:
            import gzip
            hv = gzip.open(args.hevm_gz).read()
            info = {"op_mix": "see " + args.hevm_gz}
        image = fx["packed"] if rank == 0 else np.roll(fx["packed"], 17 * rank) * (1.0 - 0.01 * rank)  # another (meaningless) image per replica
        workload = ("ResNet-20 (SiLU) HEVM program traced from the reference's examples/benchmarks/ResNet.py with its "
                    "resnet20.silu.model weights")
    else:
        prog = ha.resnet_shaped(seed=100, layers=args.layers)
        cst, hv, info = prog.assemble()
        image = np.random.default_rng(100 + rank).uniform(-0.5, 0.5, hevm.slots)
        workload = "ResNet-shaped HEVM program (SURVEY App. C op mix)"
    hevm.load_mem(cst, hv)
    for sidx in range(args.streams):
        hevm.select_stream(sidx)
        hevm.setInput(0, image)
    t_setup = time.time() - t_setup

    for _ in range(args.warmup):
        hevm.run()
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        hevm.run()  # synchronous: returns when the program has finished on the device
    barrier_sync()
    elapsed = time.perf_counter() - t0
    stats = hevm.stats()
    outs = read_outputs(hevm, args.streams) if (args.full or args.dump_outputs) else None
    rms = None
    if args.full and fx is not None:  # decrypted logits vs the torch model (examples/tests/ResNet.py:76-81: first 10 slots * 32)
        out = outs[0][0]
        rms = {"rms_vs_torch": float(np.sqrt(np.mean((out[:10] * 32 - fx["torch_result"]) ** 2))),
               "rms_vs_plaintext_evaluation": float(np.sqrt(np.mean((out - fx["expected"]) ** 2))),
               "reference_published_rms": 9.5e-4}

    ntts_per_step = ntt_equivalents(stats)
    elapsed, total_ntts = grp.job_totals(elapsed, float(ntts_per_step) * args.steps)  # max time, summed work over ranks

    if rank != 0:
        grp.close()
        return

    ms_per_step = elapsed / args.steps * 1e3
    value = total_ntts / elapsed
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, outs)
    line = {
        "metric": "NTT/s (NTT-equivalents over one run() of the ResNet HEVM program, nt=2^14)",
        "value": round(value, 1), "unit": "NTT/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "u64",
        "data": "synthetic" if fx is None else "synthetic image; weights = the reference's resnet20.silu.model",
        "config": {"workload": workload + ", nt=2^14 slots, N=2^15, 14 x 60-bit primes (SEAL_HEVM.cpp:39-53); one "
                               "independent ciphertext stream per GPU",
                   "ops": info["op_mix"], "key_switches_per_step": stats["keyswitches"], "ntt_equivalents_per_step": ntts_per_step,
                   "streams_per_gpu": args.streams,
                   "parallelism": f"replicas x{world} (no collective in the op path)", "keys": key_info},
        "hevm_wall_s": round(ms_per_step / 1e3, 4),
        "hevm_bootstrap_s_per_step": round(stats["bootstrap_s"], 4),
        "setup_s_untimed": round(t_setup, 1),
    }
    if not args.full:  # the headline only: the legs below, the decrypted-error check and the CPU baseline are --full's
        hevm.close()
        if args.out:
            print(f"[bench] full record: {emit(line, args.out)}", file=sys.stderr)
        else:
            print(json.dumps(compact_line(line)), flush=True)
        grp.close()
        return

    from dacapo_amd import progstats

    pst = progstats.walk(hv)
    # ---- the other lowerings of the same trace (same constants, same input): bootstraps to 6 and to 13 primes -------------
    lowerings = [{"boot_level": fx["meta"].get("boot_level") if fx else None, "headline": True, "ms_per_step": round(ms_per_step, 3),
                  "ntt_per_s": round(ntts_per_step * 1e3 / ms_per_step), "ntt_equivalents": pst["ntt_equivalents"],
                  "key_switch_level_histogram": pst["key_switch_level_histogram"], "opcode10": pst["opcode10_histogram"],
                  "algorithmic_bytes": pst["algorithmic_bytes"]}]
    if args.full and fx is not None and world == 1 and args.streams == 1 and not args.no_lowerings and not args.hevm_gz:
        import gzip

        for tag in ("b6", "b13"):
            f = ROOT / "tests" / "golden" / f"resnet20.{tag}.hevm.gz"
            if not f.exists():
                continue
            hv2 = gzip.open(f).read()
            hevm.load_mem(cst, hv2)
            hevm.setInput(0, image)
            hevm.run()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                hevm.run()
            dt = (time.perf_counter() - t1) / args.steps
            out2 = hevm.getOutput()[0]
            st2, p2 = hevm.stats(), progstats.walk(hv2)
            lowerings.append({"boot_level": int(tag[1:]), "headline": False, "ms_per_step": round(dt * 1e3, 3),
                              "ntt_per_s": round(st2["ntts"] / dt), "ntt_equivalents": p2["ntt_equivalents"],
                              "key_switch_level_histogram": p2["key_switch_level_histogram"], "opcode10": p2["opcode10_histogram"],
                              "algorithmic_bytes": p2["algorithmic_bytes"],
                              "achieved_gbs": round(p2["algorithmic_bytes"] / dt / 1e9, 1),
                              "rms_vs_torch": float(np.sqrt(np.mean((out2[:10] * 32 - fx["torch_result"]) ** 2)))})
    # ---- throughput mode on the reference's own key set (BEFORE the next leg adds direct rotation keys to this VM) ----------------
    streams_tab = None
    if args.full and fx is not None and world == 1 and args.streams == 1 and not args.no_streams_leg and not args.hevm_gz:
        streams_tab = streams_leg(hevm, cst, hv, image, pst["ntt_equivalents"], pst["algorithmic_bytes"], steps=max(2, args.steps))
    # ---- the same headline program with a direct Galois key for each of its rotation offsets (KeyGenerator::create_galois_keys(steps);
    # the reference's HEaaN runtime keeps such a list, HEAAN_HEVM.cpp:58-64): every rotation one key switch.  NOT the headline: the
    # reference's SEAL runtime only has the default key set (SEAL_HEVM.cpp:82-83), which the headline reproduces hop for hop.
    direct = None
    if args.full and fx is not None and world == 1 and args.streams == 1 and not args.no_lowerings and not args.hevm_gz:
        offs = sorted({(int(r) - 65536 if r >= 32768 else int(r)) for o, _, _, r in ha.unpack_hevm(hv)["ops"].tolist() if o == ha.OP_ROTATE} - {0})
        t1 = time.time()
        hevm.addRotationKeys(offs)
        t_keys = time.time() - t1
        hevm.load_mem(cst, hv)
        hevm.setInput(0, image)
        hevm.run()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            hevm.run()
        dt = (time.perf_counter() - t1) / args.steps
        out3, st3 = hevm.getOutput()[0], hevm.stats()
        direct = {"distinct_offsets": len(offs), "extra_key_bytes": len(offs) * 13 * 2 * 14 * 32768 * 8, "keygen_s": round(t_keys, 2),
                  "ms_per_step": round(dt * 1e3, 3), "key_switches_per_step": st3["keyswitches"], "ntt_equivalents_per_step": st3["ntts"],
                  "ntt_per_s": round(st3["ntts"] / dt), "rms_vs_torch": float(np.sqrt(np.mean((out3[:10] * 32 - fx["torch_result"]) ** 2)))}
    hevm.close()  # the timed VM (and its direct keys) is no longer needed: return its HBM before the other legs allocate
    ctx = ll.Context(15, 14)
    roof = roofline_leg(ll, ctx)
    # the timed step's own place on the byte roofline: SURVEY.md 8(d)'s table walked over the bytecode (progstats.walk)
    step_gbs = pst["algorithmic_bytes"] / (ms_per_step * 1e-3) / 1e9
    # the timed step's own kernels: durations, PMC traffic and (where the grid encodes level and batch) algorithmic bytes per kernel,
    # collected by tools/summarize/kernel_traffic.py on exactly this build of the library (else a note)
    top, dominant, moved = None, None, None
    tk = ROOT / "profiles" / f"{PROF}_step_kernels.json"
    if tk.exists():
        rec = json.loads(tk.read_text())
        if rec.get("lib_sha256") == lib_sha256():
            top, dominant, moved = rec.get("top_kernels"), rec.get("dominant"), rec.get("bytes_actually_moved_in_run")
        else:
            top = {"note": f"profiles/{PROF}_step_kernels.json was collected on another build"}
    folded = sum(v for k, v in pst["algorithmic_bytes_by_opcode"].items() if k in ("2", "4", "6", "7", "9"))  # negate, modswitch, addcc, addcp, mulcp
    roof["leg"] = {k: roof[k] for k in ("kernel", "achieved", "frac", "traffic", "launch")}
    roof["step"] = {"what": "one run() of the headline program", "algorithmic_bytes": pst["algorithmic_bytes"],
                    "achieved_gbs": round(step_gbs, 1), "frac": round(step_gbs / HBM_PEAK_GBS, 4),
                    "ntt_equivalents": pst["ntt_equivalents"], "bytes_by_opcode": pst["algorithmic_bytes_by_opcode"],
                    "algorithmic_bytes_of_elementwise_opcodes": folded,
                    "bytes_actually_moved": moved,
                    "bytes_actually_moved_gbs": (round(moved / (ms_per_step * 1e-3) / 1e9, 1) if moved else None),
                    "dominant": dominant, "top_kernels": top,
                    "note": "latency-bound: ~5 300 dependent launches of 4-30 us (profiles/r04_timeline.txt); most of the elementwise opcodes' "
                            "section-8(d) bytes are never moved -- the plan folds those ops into their consumers' loaders -- which is why "
                            "bytes_actually_moved (FETCH_SIZE x 2 + WRITE_SIZE over one run) is the honest numerator"}
    micro = ntt_micro_leg(ll)
    cfg3 = cfg3_leg(ll, grouped=args.full)
    per_op = per_op_leg(ll)
    ks_traffic = ks_traffic_record(per_op, cfg3)
    real_boot = real_bootstrap_leg(ll, runner) if (args.full and world == 1 and not args.no_lowerings) else None
    cpu = None
    if world == 1 and not args.no_cpu_baseline:
        hv13 = None
        if fx is not None and (ROOT / "tests" / "golden" / "resnet20.b13.hevm.gz").exists():
            import gzip

            hv13 = gzip.open(ROOT / "tests" / "golden" / "resnet20.b13.hevm.gz").read()
        cpu = cpu_baseline_leg(cst, hv, image, hv_b13=hv13 if args.full else None, openmp=args.full)

    line["config"].update(lowerings=lowerings, with_direct_rotation_keys=direct)
    line.update({
        "decrypted_error": rms,
        "roofline": roof,
        # the fed regime: S images per run() in one VM (what config 5 multiplies by the GPUs); null with --no-streams-leg / --streams > 1
        "streams": streams_tab,
        "ntt_micro": micro,
        "cfg3_mul_relin": cfg3,
        "per_op_13_primes": per_op,
        "real_bootstrap": real_boot,
        # BASELINE config 4's shape (run_s, rms_vs_torch, key switches, ...): tools/legs/resnet_real_boot.py in a child process; null under
        # --no-config4, --gpus > 1 or an external launcher
        "config4_resnet20_nt65536_N131072": config4,
        "cpu_baseline": cpu,
    })
    line["ks_traffic"] = ks_traffic
    if cpu:
        line["speedup_vs_cpu_port"] = round(value / cpu["value"], 1)
    out_path = emit(line, args.out)
    print(f"[bench] full record: {out_path}", file=sys.stderr)
    grp.close()


if __name__ == "__main__":
    main()
