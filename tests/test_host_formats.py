"""CPU-only: wire formats, assembler, C-ABI export check."""
import ctypes
import re
import struct
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_hevm_wire_format_roundtrip(tmp_path):
    from dacapo_amd import hevm_asm as ha
    from oracle.oracle import read_cst, read_hevm

    b = ha.Builder(slots=1 << 11, init_level=4)
    x = b.input(np.arange(8.0))
    y = b.add(b.rotate(x, -3), b.mul_plain(x, [1.0, 2.0]))
    y = b.mul(y, y)
    b.output(y)
    info = b.write(tmp_path / "a.cst", tmp_path / "a.hevm")
    raw = (tmp_path / "a.hevm").read_bytes()
    magic, hsize, na, nr = struct.unpack_from("<IIQQ", raw, 0)
    assert (magic, hsize, na, nr) == (0x4845564D, 24, 1, 1)  # HEVMHeader.h:10-17
    body_len, nops, nct, npt, init_level = struct.unpack_from("<5Q", raw, 24)
    assert body_len == 40 + 8 * (2 * na + 3 * nr) and init_level == 4 and nops == info["num_ops"]
    assert len(raw) == 24 + body_len + 8 * nops
    p = read_hevm(tmp_path / "a.hevm")
    assert p.arg_scale == [40] and p.arg_level == [4]
    rot = [op for op in p.ops if op[0] == 1][0]
    assert np.int16(rot[3]) == -3  # CKKSOps.td:96 : rhs carries the signed offset
    enc = [op for op in p.ops if op[0] == 0][0]
    assert enc[3] == (4 << 10) + 40  # CKKSOps.td:75
    consts = read_cst(tmp_path / "a.cst")
    assert len(consts) == 1 and consts[0].tolist() == [1.0, 2.0]
    # registers: argument 0 first, destination registers recycled
    assert p.num_ctxt <= 3 and p.res_dst[0] < p.num_ctxt
    assert np.allclose(b.expected()[0][:8], ((np.roll(np.arange(8.0)[np.arange(2048) % 8], 3) + np.arange(8.0)[np.arange(2048) % 8] * np.array([1.0, 2.0])[np.arange(2048) % 2]) ** 2)[:8])


def test_resnet_shaped_program_has_the_traced_op_mix():
    from dacapo_amd import hevm_asm as ha

    b = ha.resnet_shaped()
    cst, hv, info = b.assemble()
    mix = info["op_mix"]
    # SURVEY.md App. C targets: 2510 rotates, 4822 mulcp, 361 mulcc, ~5940 addcc, 591 addcp, 133 negates
    assert 2300 <= mix["rotate"] <= 2700 and 4200 <= mix["mulcp"] <= 5200 and 340 <= mix["mulcc"] <= 380
    assert 4000 <= mix["addcc"] <= 6500 and 550 <= mix["addcp"] <= 650 and 120 <= mix["negate"] <= 150
    assert 50 <= mix["bootstrap"] <= 200 and info["num_ctxt"] < 32  # SEAL-VM "bootstrap" = cheap re-encryption, used often


HOOKS = {"hevm_init_seeded", "hevm_init_seeded_primes", "hevm_secret_key", "hevm_test_zero_encryption"}  # csrc/test_hooks.hip


@pytest.mark.parametrize("which", ["default", "generic_width", "default_hooks", "generic_width_hooks"])
def test_library_exports_every_declared_symbol(which):
    """the C-ABI library loads without a GPU and exports everything include/*.h declares -- the default build (the reference's 60-bit chain)
    and the generic-width build of the same sources (libSEAL_HEVM_gw.so: 45..60-bit primes).  The RELEASE builds, which a maintainer copies
    next to the reference's runner, export the 18 reference symbols (SEAL_HEVM.cpp:404-504) and the safe extensions: none of the test hooks
    (the header declares those under DC_TEST_HOOKS).  The *_hooks.so builds tests/ load export exactly the four hooks more."""
    import dacapo_amd as pkg

    hooks = which.endswith("_hooks")
    path = {"default": pkg.LIB_PATH_RELEASE, "generic_width": pkg.LIB_PATH_GW_RELEASE,
            "default_hooks": pkg._LIB_DIR / "libSEAL_HEVM_hooks.so", "generic_width_hooks": pkg._LIB_DIR / "libSEAL_HEVM_gw_hooks.so"}[which]
    lib = ctypes.CDLL(str(path))

    def declared(with_hooks):
        names = set()
        for h in ("hevm_abi.h", "dacapo_ckks.h"):
            text = (ROOT / "include" / h).read_text()
            text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
            if not with_hooks:
                text = re.sub(r"#ifdef DC_TEST_HOOKS.*?#endif", "", text, flags=re.S)
            text = re.sub(r"^\s*#.*$", "", text, flags=re.M)          # preprocessor lines (#pragma GCC visibility push(default))
            names |= set(re.findall(r"\b(\w+)\s*\([^;{]*\)\s*;", text))
        return names - {"defined"}

    names = declared(hooks)
    assert declared(True) - declared(False) == HOOKS
    reference_18 = {"initFullVM", "initClientVM", "initServerVM", "create_context", "load", "loadClient", "encrypt", "decrypt",
                    "decrypt_result", "getResIdx", "getCtxt", "preprocess", "run", "getArgLen", "getResLen", "setDebug",
                    "setToGPU", "printMem"}
    assert reference_18 <= names and len(names) >= 18 + 25
    for n in sorted(names):
        assert hasattr(lib, n), n
    # ... and NOTHING else: -fvisibility=hidden + csrc/exports.map (round 3's library exported ~250 dacapo:: C++ symbols next to these)
    import subprocess

    nm = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert exported == names, (sorted(exported - names), sorted(names - exported))
    assert bool(exported & HOOKS) == hooks and (not hooks or HOOKS <= exported)
    listed = set(re.findall(r"^\s+(\w+);", (ROOT / "dacapo_amd" / "csrc" / "exports.map").read_text(), flags=re.M))
    assert listed == declared(False) and not (listed & HOOKS)  # exports.map is the release list; the Makefile derives the hooks list from it


def test_tests_run_on_the_hooks_build_and_everything_else_on_the_release_build():
    """tests/conftest.py selects the hooks builds for this process; a process without DACAPO_AMD_HOOKS -- bench.py, smoke(), a maintainer's
    runner -- binds the release build, where HEVM(seed=...) fails loudly instead of falling back"""
    import os
    import subprocess
    import sys

    import dacapo_amd as pkg

    assert pkg.HOOKS and pkg.LIB_PATH.name == "libSEAL_HEVM_hooks.so" and pkg.LIB_PATH_GW.name == "libSEAL_HEVM_gw_hooks.so"
    env = {k: v for k, v in os.environ.items() if k != "DACAPO_AMD_HOOKS"}
    code = ("import sys; sys.path.insert(0, %r); import dacapo_amd as p; from dacapo_amd import runner; L = runner.reinit_lw();"
            "print(p.LIB_PATH.name, p.LIB_PATH_GW.name, L.has_test_hooks)" % str(ROOT))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["libSEAL_HEVM.so", "libSEAL_HEVM_gw.so", "False"], out.stderr[-500:]


def test_options_come_from_one_environment_variable(tmp_path):
    """a caller that only knows the reference's 18 symbols configures the library through ONE environment variable,
    DACAPO_HEVM_OPTIONS="name=value,..." (csrc/options.hpp), parsed the first time an option is read; a mistyped name aborts with the list
    of names instead of silently running the default.  Host-only: no GPU call."""
    import subprocess
    import sys

    code = ("import ctypes, sys; sys.path.insert(0, %r); from dacapo_amd import runner; L = runner.reinit_lw();"
            "print(L.hevm_get_option(b'logn'), L.hevm_get_option(b'primes'), L.hevm_get_option(b'plan'), L.hevm_get_option(b'sum_pair_min_wgs'))" % str(ROOT))
    import os

    env = dict(os.environ, DACAPO_HEVM_OPTIONS="logn=12,primes=4,sum_pair_min_wgs=0")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["12", "4", "1", "0"], out.stderr[-500:]
    env = dict(os.environ, DACAPO_HEVM_OPTIONS="logn=12,primse=4")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "unknown option" in out.stderr and "primes" in out.stderr
    # a malformed VALUE aborts too (round-4 advisor: "plan=" used to run as 0, "max_batch=12abc" as 12, "seal_compr=zlib" as none)
    for bad in ("plan=", "max_batch=12abc", "logn=twelve", "primes=4 "):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DACAPO_HEVM_OPTIONS=bad), capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "needs an integer value" in out.stderr, (bad, out.stderr[-300:])
    code2 = code.replace("b'sum_pair_min_wgs'", "b'seal_compr'")
    out = subprocess.run([sys.executable, "-c", code2], env=dict(os.environ, DACAPO_HEVM_OPTIONS="seal_compr=zstd,plan=0x0"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["15", "14", "0", "2"], out.stderr[-300:]   # the names of include/hevm_abi.h; hex integers
    # the per-knob variables of rounds 1-3 are no longer read: setting one is named in a warning instead of silently running the defaults
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DACAPO_HEVM_LOGN="12", DACAPO_KS_SPECIAL="4"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split()[0] == "15" and "DACAPO_HEVM_LOGN is no longer read" in out.stderr and "DACAPO_KS_SPECIAL" in out.stderr


def test_outputs_keep_their_registers_when_used_afterwards():
    from dacapo_amd import hevm_asm as ha
    from oracle.oracle import read_hevm
    import tempfile

    b = ha.Builder(slots=1 << 11, init_level=4)
    x = b.input(np.arange(4.0))
    p = b.mul_plain(x, [2.0])
    b.output(p)                      # declared an output, then still used
    q = b.add_plain(b.negate(p), [1.0])
    b.output(q)
    cst, hv, info = b.assemble()
    with tempfile.NamedTemporaryFile(suffix=".hevm") as f:
        f.write(hv)
        f.flush()
        prog = read_hevm(f.name)
    assert len(set(prog.res_dst)) == 2
    writes_after = [op for op in prog.ops[[i for i, o in enumerate(prog.ops) if o[0] == 9][0] + 1:] if op[0] != 0 and op[1] == prog.res_dst[0]]
    assert not writes_after  # nothing overwrites the first result's register


def test_headers_are_plain_c_and_link_against_the_library(tmp_path):
    """the drop-in boundary is a C ABI: include/*.h compile as C99 (no C++ or torch types in any signature) and a C caller
    that references every declared function links against dacapo_amd/lib/libSEAL_HEVM.so (no GPU needed to link)"""
    import re
    import shutil
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    lib = root / "dacapo_amd" / "lib" / "libSEAL_HEVM.so"
    if not lib.exists() or not shutil.which("gcc"):
        import pytest

        pytest.skip("library not built or no gcc")
    names = []
    for h in ("hevm_abi.h", "dacapo_ckks.h"):
        text = re.sub(r"#ifdef DC_TEST_HOOKS.*?#endif", "", (root / "include" / h).read_text(), flags=re.S)  # the release library: no test hooks
        names += re.findall(r"^[A-Za-z_][\w \*]*?\b(\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M)
    names = sorted({n for n in names if n not in ("defined", "if", "sizeof")})
    assert len(names) >= 50 and "initFullVM" in names and "dc_ntt_forward" in names
    src = '#include "hevm_abi.h"\n#include "dacapo_ckks.h"\nvoid *table[] = {\n' + "".join(f"    (void *){n},\n" for n in names) + "};\n"
    src += "int main(void) { return sizeof(table) == 0; }\n"
    (tmp_path / "c.c").write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-pedantic", f"-I{root / 'include'}", "-c", str(tmp_path / "c.c"), "-o",
                           str(tmp_path / "c.o")])
    subprocess.check_call(["gcc", str(tmp_path / "c.o"), f"-L{lib.parent}", "-lSEAL_HEVM", "-Wl,--unresolved-symbols=ignore-in-shared-libs",
                           "-o", str(tmp_path / "c")])


def _ref_wire():
    from pathlib import Path

    p = Path(__file__).resolve().parent.parent / "oracle" / "_ref" / "hevm_wire_ref"
    return p if p.exists() else None


# what oracle/_ref/hevm_wire_ref printed for _wire_images() (tools/fixtures/record_wire_ref.py): the reference reader's view of the same bytes,
# for a checkout built where the reference is not readable
WIRE_REF = ROOT / "tests" / "golden" / "hevm_wire_ref.json"


def _wire_images():
    """name -> .hevm bytes: the traced fixtures and two hand-assembled programs"""
    import gzip

    from dacapo_amd import hevm_asm as ha

    golden = ROOT / "tests" / "golden"
    images = {p.name: gzip.open(p).read() for p in sorted(golden.glob("*.hevm.gz")) + sorted((golden / "suite").glob("*.hevm.gz"))}
    rng = np.random.default_rng(3)
    images["sobel"] = ha.sobel_filter(rng.uniform(0, 1, 4096), slots=4096, init_level=6).assemble()[1]
    images["linreg"] = ha.linear_regression(rng.uniform(-1, 1, 4096), rng.uniform(-1, 1, 4096), slots=4096, init_level=12).assemble()[1]
    return images


def test_wire_format_against_the_reference_header(tmp_path):
    """oracle/_ref/hevm_wire_ref is built from the reference's own include/hecate/Support/HEVMHeader.h (the one source of
    its HEVM path that compiles here) and reads a .hevm file in the order SEAL_HEVM::loadHEVM does (SEAL_HEVM.cpp:202-234).
    What it sees must be what our assembler wrote and what our reader returns -- for hand-assembled programs and for the
    traced fixtures.  Where the binary is not built, its recorded output (tests/golden/hevm_wire_ref.json, keyed by the
    sha256 of the bytes it read) stands in for it; where it is, live and recorded output must agree."""
    import hashlib
    import json
    import subprocess

    from dacapo_amd import hevm_asm as ha

    exe = _ref_wire()
    recorded = json.loads(WIRE_REF.read_text())
    layout = json.loads(subprocess.check_output([str(exe)])) if exe else recorded["layout"]
    assert layout == recorded["layout"]
    assert (layout["sizeof_HEVMHeader"], layout["sizeof_ConfigBody"], layout["sizeof_HEVMOperation"]) == (24, 40, 8)
    assert layout["default_magic"] == ha.MAGIC and layout["offsetof_arg_length"] == 8 and layout["offsetof_init_level"] == 32
    images = _wire_images()
    assert len(images) >= 9
    for name, raw in images.items():
        rec = recorded["images"].get(name)
        if exe:
            (tmp_path / "p.hevm").write_bytes(raw)
            ref = json.loads(subprocess.check_output([str(exe), str(tmp_path / "p.hevm")]))
            if rec is not None and rec["sha256"] == hashlib.sha256(raw).hexdigest():
                assert ref == rec["reader"], name
        else:
            assert rec is not None, f"{name}: no recorded reader output (tools/fixtures/record_wire_ref.py)"
            assert rec["sha256"] == hashlib.sha256(raw).hexdigest(), f"{name}: bytes differ from the recorded ones (tools/fixtures/record_wire_ref.py)"
            ref = rec["reader"]
        ours = ha.unpack_hevm(raw)
        assert ref["complete"] and ref["at_end"], name  # the reference reader consumes the file exactly
        assert ref["magic_number"] == ha.MAGIC and ref["hevm_header_size"] == 24
        assert ref["config_body_length"] == 40 + 8 * (2 * len(ours["arg_scale"]) + 3 * len(ours["res_scale"]))
        for k in ("arg_scale", "arg_level", "res_scale", "res_level", "res_dst", "num_ctxt", "num_ptxt", "init_level"):
            assert ref[{"num_ctxt": "num_ctxt_buffer", "num_ptxt": "num_ptxt_buffer"}.get(k, k)] == ours[k], (name, k)
        assert ref["num_operations"] == len(ours["ops"])
        h = 1469598103934665603
        for w in ours["ops"].ravel().tolist():
            h = ((h ^ w) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        assert ref["ops_fnv1a"] == h, name
        assert ref["op_counts"][:11] == [int((ours["ops"][:, 0] == k).sum()) for k in range(11)]


def test_boundary_matches_the_reference_callers_bindings():
    """tests/golden/runner_bindings.json = what the reference's Python driver binds with ctypes (runner.py:34-71, extracted
    by tools/fixtures/extract_runner_bindings.py).  Every one of those 18 symbols is exported by the library and declared in
    include/hevm_abi.h with a parameter list of the same length and compatible C types, result included."""
    import json

    spec = json.loads((ROOT / "tests" / "golden" / "runner_bindings.json").read_text())["bindings"]
    assert len(spec) == 18
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hevm_abi.h").read_text(), flags=re.S)
    lib = ctypes.CDLL(str(ROOT / "dacapo_amd" / "lib" / "libSEAL_HEVM.so"))
    ctype_of = {"c_char_p": {"char *", "const char *"}, "c_bool": {"bool"}, "c_void_p": {"void *", "struct hevm_ctxt *", "const void *"},
                "c_int64": {"int64_t"}, "c_int": {"int", "void"}, "POINTER(c_double)": {"double *", "const double *"}}
    for name, b in spec.items():
        assert hasattr(lib, name), name
        m = re.search(r"^([\w \*]+?)\b" + name + r"\s*\(([^)]*)\)\s*;", header, flags=re.M)
        assert m, f"{name} not declared in include/hevm_abi.h"
        ret = m.group(1).strip()
        params = [re.sub(r"\s*\b\w+$", "", p.strip()).strip() for p in m.group(2).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(b["argtypes"]), (name, params, b["argtypes"])
        for have, want in zip(params, b["argtypes"]):
            assert have.replace(" *", " *") in ctype_of[want], (name, have, want)
        assert ret in ctype_of[b["restype"]], (name, ret, b["restype"])


def test_instruction_encoding_matches_the_reference_emitter():
    """tests/golden/opcode_table.json = opcode number and operand-field kinds per CKKS op as the reference's emitter writes
    them (CKKSOps.td:60-222, extracted by tools/fixtures/extract_opcode_table.py); the assembler uses the same numbers and packs the
    same fields, and the VM's dispatch (via the op-count statistics of an assembled program) agrees."""
    import json

    from dacapo_amd import hevm_asm as ha

    ops = json.loads((ROOT / "tests" / "golden" / "opcode_table.json").read_text())["ops"]
    want = {"encode": ha.OP_ENCODE, "rotatec": ha.OP_ROTATE, "negatec": ha.OP_NEGATE, "rescalec": ha.OP_RESCALE, "modswitchc": ha.OP_MODSWITCH,
            "upscalec": ha.OP_UPSCALE, "addcc": ha.OP_ADDCC, "addcp": ha.OP_ADDCP, "mulcc": ha.OP_MULCC, "mulcp": ha.OP_MULCP,
            "bootstrapc": ha.OP_BOOTSTRAP}
    assert set(ops) == set(want)
    for name, num in want.items():
        assert ops[name]["opcode"] == num, name
    assert ops["encode"]["rhs"] == "imm:(getLevel()<<10)+getScale()" and ops["encode"]["dst"] == "plain"
    assert ops["addcp"]["rhs"] == ops["mulcp"]["rhs"] == "plain" and ops["addcc"]["rhs"] == ops["mulcc"]["rhs"] == "cipher"
    assert ops["bootstrapc"]["rhs"] == "imm:getLevel()" and ops["modswitchc"]["rhs"] == "imm:getDownFactor()"
    # the assembler packs exactly those fields
    b = ha.Builder(slots=64, init_level=5)
    x = b.input(np.zeros(64))
    y = b.bootstrap(b.modswitch(b.rescale(b.mul_plain(b.add_plain(b.negate(b.rotate(x, -3)), [1.0]), [2.0], scale_bits=60, normalise=False)), 1), 4)
    b.output(b.add(b.mul(y, y), b.mul(y, y)))
    wire = ha.unpack_hevm(b.assemble()[1])["ops"]
    by = {int(r[0]): r for r in wire[::-1]}  # one example of each opcode
    assert int(by[ha.OP_ENCODE][3]) >> 10 == 5 and int(by[ha.OP_ROTATE][3]) == 0xFFFD and int(by[ha.OP_MODSWITCH][3]) == 1
    assert int(by[ha.OP_BOOTSTRAP][3]) == 4 and int(by[ha.OP_NEGATE][3]) == 0 and int(by[ha.OP_RESCALE][3]) == 0
    assert int(by[ha.OP_ADDCP][3]) < b.num_plain and int(by[ha.OP_MULCP][3]) < b.num_plain


def test_every_tool_a_script_or_document_names_exists():
    """tools/ is measurement and fixture plumbing in four directories (tools/README.md); the collection scripts, bench.py, the tests and the
    current documents name its files by path -- every such path must exist (the round-5 reorganisation moved 29 of them)."""
    import re

    names = set()
    files = list((ROOT / "tools").glob("*.sh")) + [ROOT / "bench.py", ROOT / "DESIGN.md", ROOT / "INTEGRATION.md", ROOT / "README.md", ROOT / "tools" / "README.md",
                                                    ROOT / "docs" / "rounds" / "r05.md", ROOT / "tools" / "profiles_readme.py"] + list((ROOT / "tests").glob("*.py"))
    for f in files:
        for m in re.finditer(r"tools/(?:[a-z_]+/)?[A-Za-z0-9_]+\.(?:py|sh|cpp|hip)", f.read_text()):
            names.add(m.group(0))
    assert len(names) > 30
    missing = sorted(n for n in names if not (ROOT / n).exists())
    assert not missing, missing
    for sub in ("legs", "summarize", "fixtures", "experiments"):
        assert (ROOT / "tools" / sub).is_dir()
    # a tool two levels below the root finds the root two levels up (parents[2] / .parent.parent.parent), not one
    for sub in ("legs", "summarize", "fixtures"):
        for f in (ROOT / "tools" / sub).glob("*.py"):
            t = f.read_text()
            assert not re.search(r"__file__\)\.resolve\(\)\.parents\[1\]", t), f
            assert not re.search(r"__file__\)\.resolve\(\)\.parent\.parent(?!\.parent)", t), f
