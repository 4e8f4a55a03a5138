#!/usr/bin/env python3
"""Record what oracle/_ref/hevm_wire_ref (the reference's wire-format header, compiled by oracle/Makefile) prints for the .hevm images of
tests/test_host_formats.py::test_wire_format_against_the_reference_header, so that the test runs where the binary cannot be built.
Each image's entry carries the sha256 of the bytes the reader was given.  Run it again whenever a fixture or the assembler changes:

    python tools/fixtures/record_wire_ref.py > tests/golden/hevm_wire_ref.json
"""
import hashlib
import importlib.util
import json
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def main():
    spec = importlib.util.spec_from_file_location("test_host_formats", ROOT / "tests" / "test_host_formats.py")
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    exe = t._ref_wire()
    if exe is None:
        sys.exit("oracle/_ref/hevm_wire_ref is not built (make -C oracle where the reference's header is readable)")
    out = {"source": "output of oracle/_ref/hevm_wire_ref (oracle/ref_wire.cpp over the reference's HEVMHeader.h); "
                     "tools/fixtures/record_wire_ref.py",
           "layout": json.loads(subprocess.check_output([str(exe)])), "images": {}}
    with tempfile.TemporaryDirectory() as d:
        f = Path(d) / "p.hevm"
        for name, raw in t._wire_images().items():
            f.write_bytes(raw)
            out["images"][name] = {"sha256": hashlib.sha256(raw).hexdigest(), "reader": json.loads(subprocess.check_output([str(exe), str(f)]))}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
