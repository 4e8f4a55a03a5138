"""The launch rule of the SEAL-layout key switch (dacapo_amd/csrc/launch_shape.hpp) on its own, without a GPU.

`make -C dacapo_amd/csrc launch_shape_asan` builds the header with the option table (options.cpp) and a small driver (launch_shape_main.cpp)
under AddressSanitizer + UBSan.  The driver prints, per case (logN, hybrid, B, ell), the five answers

    big fused_mac folds_rescale carries_addend chain_fusion

that the launchers, the plan and the C entry points all take from this one place.  Every expected line below is a literal worked out from the
rule and the option defaults, never from the code under test:

    tiles          = (N / 1024) * B * ell^2
    big            = tiles >= ks_big_tiles                      (default 4096)
    fused_mac      = ks_fuse_mac and tiles < ks_fuse_mac_tiles  (defaults 1 and 2^40)
    folds_rescale  = not hybrid and ell >= 2 and fused_mac and not big
    carries_addend = not hybrid and fused_mac
    chain_fusion   = ks_fuse_mac and ks_fuse_mac_tiles == 2^40

In particular the forbidden pair -- an addend on a batch whose middle is not one launch, which b_rotate_hops answers with an abort -- is
covered here (carries_addend is 0 on that side) and never run on a GPU."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dacapo_amd" / "csrc"
DRIVER = CSRC / "build_asan" / "launch_shape_asan"


@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no g++ / make")
    r = subprocess.run(["make", "-C", str(CSRC), "launch_shape_asan"], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()) and "error:" not in r.stderr:
        pytest.skip("this toolchain has no AddressSanitizer runtime: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-2000:]
    return DRIVER


# (options, [((logN, hybrid, B, ell), "big fused_mac folds_rescale carries_addend chain_fusion")])
CASES = [
    ("", [  # N = 2^12, ell = 3: tiles = 36 B, on either side of 4096
        ((12, 0, 113, 3), "0 1 1 1 1"),   # 4068
        ((12, 0, 114, 3), "1 1 0 1 1"),   # 4104
        # N = 2^15: tiles = 32 B ell^2
        ((15, 0, 1, 11), "0 1 1 1 1"),    # 3872
        ((15, 0, 2, 11), "1 1 0 1 1"),    # 7744
        ((15, 0, 1, 13), "1 1 0 1 1"),    # 5408
        # ell = 1: no rescale to fold, at any size
        ((12, 0, 1, 1), "0 1 0 1 1"),     # 4
        ((15, 0, 200, 1), "1 1 0 1 1"),   # 6400
        # grouped digits: no fold, no addend, at any size (big and fused_mac are the bare thresholds)
        ((12, 1, 1, 3), "0 1 0 0 1"),
        ((12, 1, 114, 3), "1 1 0 0 1"),
        ((15, 1, 1, 11), "0 1 0 0 1"),
    ]),
    ("ks_fuse_mac_tiles=72", [  # N = 2^12, ell = 3; no chain fusion once the threshold is set
        ((12, 0, 1, 3), "0 1 1 1 0"),     # 36: fused, carries an addend
        ((12, 0, 2, 3), "0 0 0 0 0"),     # 72: not fused, no addend, no fold
    ]),
    ("ks_fuse_mac=0", [  # nothing fused, nothing folds, no addend, no chain fusion, at any size
        ((12, 0, 1, 3), "0 0 0 0 0"),
        ((12, 0, 114, 3), "1 0 0 0 0"),
        ((15, 0, 2, 11), "1 0 0 0 0"),
        ((12, 1, 1, 3), "0 0 0 0 0"),
    ]),
    ("ks_big_tiles=1", [  # every batch takes the large-batch sequence: the middle stays fused, the fold goes
        ((12, 0, 1, 3), "1 1 0 1 1"),
    ]),
    ("ks_big_tiles=36,ks_fuse_mac_tiles=37", [  # both thresholds at the batch's own 36 tiles: >= for big, < for the fused middle
        ((12, 0, 1, 3), "1 1 0 1 0"),
    ]),
]


@pytest.mark.parametrize("options,cases", CASES, ids=[c[0] or "defaults" for c in CASES])
def test_launch_rule(driver, options, cases):
    env = {k: v for k, v in os.environ.items() if k != "DACAPO_HEVM_OPTIONS"}
    if options:
        env["DACAPO_HEVM_OPTIONS"] = options
    args = [str(v) for case, _ in cases for v in case]
    r = subprocess.run([str(driver), *args], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])  # (a sanitizer report is a non-zero exit and text on stderr)
    got = r.stdout.splitlines()
    assert len(got) == len(cases), r.stdout
    for (case, want), line in zip(cases, got):
        assert line == want, (options, case, line, want)
