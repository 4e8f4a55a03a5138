#!/usr/bin/env python3
"""Real CKKS bootstrapping on the MI355X: one ciphertext at 1 prime -> `target` primes, through the extension opcodes and
dacapo_amd/ckks_boot.py.   python tools/legs/boot_demo.py [logN=15] [r=5] [direct_keys=1] [target=3] [ks_special=1] [ks_alpha=ks_special] [--opt name=value ...]
ks_special > 1: grouped-digit hybrid key switching (hybrid_ks.hip), the chain gets that many special primes.
BASELINE config 4's geometry: python tools/legs/boot_demo.py 17 5 1 14 8 7
--sse <main weight>:<ephemeral weight> (e.g. 0:32 = SEAL's dense secret): sparse-secret encapsulation (options secret_hw / boot_secret_hw, opcode
20 around ModRaise); without it the keys are generated under a weight-64 secret.
--real-msg: the half bootstrap for real messages (ckks_boot.BootstrapEmitter(real_msg=True): one EvalMod, one SlotToCoeff chain).
--forms full,half,full: several programs one after the other in ONE process and one VM (the full form's rotation keys serve both).
The last line is a JSON record, one entry per form run (field real_msg)."""
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from dacapo_amd import ckks_boot as cb  # noqa: E402
from dacapo_amd import hevm_asm as ha  # noqa: E402
from dacapo_amd import runner  # noqa: E402

sse_weights = None
if "--sse" in sys.argv:
    i = sys.argv.index("--sse")
    sse_weights = tuple(int(w) for w in sys.argv[i + 1].split(":"))
    assert len(sse_weights) == 2 and sse_weights[1] > 0, "--sse <main weight>:<ephemeral weight>"
    del sys.argv[i:i + 2]
forms = ["half" if "--real-msg" in sys.argv else "full"]
if "--real-msg" in sys.argv:
    sys.argv.remove("--real-msg")
if "--forms" in sys.argv:
    i = sys.argv.index("--forms")
    forms = sys.argv[i + 1].split(",")
    assert forms and all(f in ("full", "half") for f in forms), "--forms full,half,..."
    del sys.argv[i:i + 2]
sys.argv = runner.apply_cli_options(sys.argv)
logN = int(sys.argv[1]) if len(sys.argv) > 1 else 15
r = int(sys.argv[2]) if len(sys.argv) > 2 else 5
direct = int(sys.argv[3]) if len(sys.argv) > 3 else 1
target = int(sys.argv[4]) if len(sys.argv) > 4 else 3
ks = int(sys.argv[5]) if len(sys.argv) > 5 else 1
alpha = int(sys.argv[6]) if len(sys.argv) > 6 else ks
progs = {f: cb.single_bootstrap_program(logN, target=target, r=r, ks=ks, sse=sse_weights is not None, real_msg=f == "half") for f in set(forms)}
K = next(iter(progs.values()))[0]
slots = 1 << (logN - 1)
print(f"{'SSE: main secret weight %d (0: dense), ephemeral %d' % sse_weights if sse_weights else 'secret weight 64'}")
msg = np.random.default_rng(3).uniform(-1, 1, slots)
t0 = time.time()
hevm = runner.HEVM(fresh=True, logN=logN, num_primes=K, ks_special=ks, ks_alpha=alpha, vm_options={"secret_hw": 64} if sse_weights is None else {"secret_hw": sse_weights[0], "boot_secret_hw": sse_weights[1]})
print(f"context + keys: {time.time()-t0:.1f} s")
if direct:
    offs = sorted(set().union(*[p[3] for p in progs.values()]))  # (the half form's offsets are a subset of the full form's)
    t0 = time.time()
    hevm.addRotationKeys(offs)
    print(f"{len(offs)} direct rotation keys: {time.time()-t0:.1f} s")
records = []
for form in forms:
    _, cst, hv, _, em = progs[form]
    info = {'num_ops': len(ha.unpack_hevm(hv)['ops']), 'num_ptxt': ha.unpack_hevm(hv)['num_ptxt']}
    print(f"[{form}] N=2^{logN}, {K} primes ({ks} special), target {target}, r={r}: {info['num_ops']} instructions, {info['num_ptxt']} plaintexts, {len(cst)/1e6:.0f} MB of constants")
    sim = cb.simulate(hv, cst, [msg], logN, em.primes)[0]
    print("cleartext simulation: max error", np.abs(sim - msg).max())
    t0 = time.time()
    hevm.load_mem(cst, hv)
    print(f"load + preprocess: {time.time()-t0:.1f} s")
    hevm.setInput(0, msg)
    hevm.run()
    for _ in range(2):
        t0 = time.perf_counter()
        hevm.run()
        dt = time.perf_counter() - t0
    out = hevm.getOutput()[0]
    err = np.abs(out - msg)
    st = hevm.stats()
    c = hevm.getCtxt(hevm.getResIdx(0))
    print(f"bootstrap: {dt*1e3:.2f} ms, {st['keyswitches']} key switches, {st['ntts']} NTT-equivalents, result at {c.level} primes, scale 2^{np.log2(c.scale):.3f}")
    print(f"decrypted vs message: max error {err.max():.3e}, rms {np.sqrt(np.mean(err**2)):.3e}  ({-np.log2(err.max()):.1f} bits)")
    records.append({"real_msg": form == "half", "N": 1 << logN, "primes": K, "special_primes": ks, "primes_per_digit": alpha, "target": target,
                    "instructions": info["num_ops"], "plaintexts": info["num_ptxt"], "plaintext_bytes": hevm.plaintextBytes(),
                    "bootstrap_ms": round(dt * 1e3, 3), "key_switches": st["keyswitches"], "ntt_equivalents": st["ntts"],
                    "max_error": float(err.max()), "rms_error": float(np.sqrt(np.mean(err**2))), "bits": round(float(-np.log2(err.max())), 2),
                    "simulate_max_error": float(np.abs(sim - msg).max())})
print(json.dumps({"sse": list(sse_weights) if sse_weights else None, "runs": records}))
