"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` is the headline alone -- set-up, W warm-up steps, K timed steps, the result line --
and `--dump-outputs DIR` writes what the last timed step computed: the decrypted result of the ResNet-20 program, checked here against the
plaintext evaluation and the torch model (the checks a plain run leaves to --full).  bench.py runs as a CHILD process on the release build."""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")


def test_plain_run_is_the_headline_alone_and_dumps_the_decrypted_result(tmp_path):
    from dacapo_amd import hevm_asm as ha

    env = dict(os.environ)
    env.pop("DACAPO_AMD_HOOKS", None)  # bench.py runs on the RELEASE build of the library
    steps, warmup = 3, 1
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "out")]
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(ROOT))
    wall = time.time() - t0
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and r.stdout.strip().splitlines()[-1] == lines[0]
    line = json.loads(lines[0])
    for k in CONTRACT:
        assert k in line, k
    assert line["steps"] == steps and line["warmup"] == warmup and line["n_gpus"] == 1
    assert line["unit"] == "NTT/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(line["config"]["ntt_equivalents_per_step"] / (line["ms_per_step"] * 1e-3), rel=1e-3)
    for k in ("roofline", "cpu_baseline", "config4", "speedup_vs_cpu_port"):
        assert k not in line, k
    assert line["rms_vs_torch"] is None and line["cfg3_us"] is None and line["full_record"] is None
    assert "full record" not in r.stderr
    assert wall - (steps + warmup) * line["ms_per_step"] * 1e-3 < 30.0, wall

    fx = ha.read_fixture(ROOT / "tests" / "golden" / "resnet20")
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["output.npy"]
    out = np.load(tmp_path / "out" / "output.npy")
    assert out.dtype == np.float64 and out.ndim == 2 and out.shape[1] == fx["expected"].shape[0]
    assert float(np.sqrt(np.mean((out[0] - fx["expected"]) ** 2))) < 1e-5
    assert float(np.sqrt(np.mean((out[0][:10] * 32 - fx["torch_result"]) ** 2))) < 2e-3
