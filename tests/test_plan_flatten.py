"""The flattening pass of rotate-and-add chains (dacapo_amd/csrc/plan_flatten.cpp; option ks_flatten_sums) on its own, without a GPU.

`make -C dacapo_amd/csrc plan_groups_asan` builds the pass -- host-only C++, plain arrays in, groups out --, the library's walk of a program
(plan_flow.cpp) and a small driver (plan_groups_main.cpp) under AddressSanitizer + UBSan.  `plan_groups_asan flatten` reads a .hevm program,
walks it as the library does and prints the groups: stages of a chain
y' = y + rotate(y, o) that one hoisted lazy sum with an addend computes (2^h - 1 rotations of the stage's first y, plus that y).

  * the committed programs at f = 2, 3, 6: the driver's groups equal those of `flatten_groups` below, a restatement of the rules written here
    from their description (csrc/plan_flatten.hpp) and sharing no code with the pass; the counts of the headline program are pinned;
  * hand-made programs: an interior value with a third reader, an interior value that is a result, a rotation read twice, either operand
    order of the add, a subset sum that is 0 modulo the slot count, a missing key in the middle of a chain, 7 hops at f = 3 (3 + 2 + 2);
  * the sanitizers stay silent (-fno-sanitize-recover: a finding is a non-zero exit status and text on stderr)."""
import gzip
import json
import shutil
import subprocess
from pathlib import Path

import pytest

from dacapo_amd import hevm_asm as ha

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dacapo_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden"
DRIVER = CSRC / "build_asan" / "plan_groups_asan"

ROT, NEG, RESCALE, MODSWITCH, ADDCC, ADDCP, MULCC, MULCP, BOOT = 1, 2, 3, 4, 6, 7, 8, 9, 10
UNARY = {ROT, NEG, RESCALE, MODSWITCH, ADDCP, MULCP, BOOT, 17, 18, 19, 20}
BINARY = {ADDCC, MULCC}


def s16(x):
    x = int(x) & 0xFFFF
    return x - 0x10000 if x >= 0x8000 else x


def norm_offset(o, slots):
    """the representative of o modulo slots in (-slots / 2, slots / 2]"""
    o %= slots
    return o - slots if o > slots // 2 else o


def flatten_groups(ops, res_dst, f, slots, keyed=None):
    """The rules of csrc/plan_flatten.hpp, restated: [(closing op, source value, [(rotate op, addcc op), ...], [member offset, ...]), ...] in
    the order of the closing ops.  A value is the index of the instruction that wrote it, or -1 - r for input register r.  keyed: the
    offsets that have a key (None: all)."""
    cur = {}
    readers, insts = {}, {}
    for i, (opc, dst, lhs, rhs) in enumerate([tuple(int(x) for x in op) for op in ops]):
        if opc not in UNARY and opc not in BINARY:
            continue
        if opc == MODSWITCH and s16(rhs) <= 0:
            continue
        if opc == ROT and s16(rhs) == 0 and dst == lhs:
            continue
        srcs = [cur.get(lhs, -1 - lhs)] + ([cur.get(rhs, -1 - rhs)] if opc in BINARY else [])
        for v in srcs:
            readers[v] = readers.get(v, 0) + 1
        insts[i] = (opc, srcs, s16(rhs))
        cur[dst] = i
    results = {cur[r] for r in res_dst if r in cur}
    keyed = None if keyed is None else {norm_offset(o, slots) for o in keyed}
    hidden = lambda v: v not in results
    # hops: addcc i = y + a with a = rotate(y, o) read by nothing else and unobservable
    hop = {}
    for i, (opc, srcs, _) in insts.items():
        if opc != ADDCC:
            continue
        for y, a in (srcs, srcs[::-1]):
            if a in insts and insts[a][0] == ROT and insts[a][1][0] == y and readers.get(a, 0) == 1 and hidden(a):
                hop[i] = (a, y)
                break
    follows = {}  # previous hop's addcc -> the hop that continues from it
    for i, (a, y) in hop.items():
        if y in hop and readers.get(y, 0) == 2 and hidden(y):
            follows[y] = i
    groups = []
    for head in sorted(set(hop) - set(follows.values())):
        chain = [head]
        while chain[-1] in follows:
            chain.append(follows[chain[-1]])
        m = len(chain)
        stages = -(-m // f)
        sizes = [m // stages + (1 if s < m % stages else 0) for s in range(stages)]
        at = 0
        for h in sizes:
            stage, at = chain[at:at + h], at + h
            if h < 2:
                continue
            offs = [insts[hop[i][0]][2] for i in stage]
            members = [norm_offset(sum(o for k, o in enumerate(offs) if mask >> k & 1), slots) for mask in range(1, 1 << h)]
            if any(o == 0 for o in members) or (keyed is not None and any(o not in keyed for o in members)):
                continue
            groups.append((stage[-1], hop[stage[0]][1], [(hop[i][0], i) for i in stage], members))
    return sorted(groups)


def totals(groups):
    """(groups, hops absorbed, members, distinct offsets, distinct offsets that are no single hop's)"""
    every = {o for g in groups for o in g[3]}
    single = {g[3][(1 << k) - 1] for g in groups for k in range(len(g[2]))}
    return len(groups), sum(len(g[2]) for g in groups), sum(len(g[3]) for g in groups), len(every), len(every - single)


@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no g++ / make")
    r = subprocess.run(["make", "-C", str(CSRC), "plan_groups_asan"], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()) and "error:" not in r.stderr:
        pytest.skip("this toolchain has no AddressSanitizer runtime: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-2000:]
    return DRIVER


def groups_of(driver, hevm_path, f, slots, keyed=None):
    """(rotate instructions, groups as flatten_groups gives them) as the driver prints them; stderr must be empty"""
    cmd = [str(driver), "flatten", str(hevm_path), str(f), str(slots)] + ([",".join(str(o) for o in sorted(keyed))] if keyed is not None else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    head = lines[0].split()
    assert head[0::2] == ["rotates", "groups", "hops", "members", "offsets", "composite"]
    out = []
    for line in lines[1:]:
        left, hops, members = line.split(":")
        w = left.split()
        assert w[0] == "group" and w[1] == "closing" and w[3] == "source" and w[5] == "hops"
        pairs = [tuple(int(x) for x in p.split("/")) for p in hops.split()]
        assert len(pairs) == int(w[6])
        out.append((int(w[2]), int(w[4]), pairs, [int(o) for o in members.split()]))
    assert tuple(int(x) for x in head[3::2]) == totals(out)
    return int(head[1]), out


FIXTURES = ["resnet20", "resnet20.b13", "resnet20.b6", "resnet20_nt16", "resnet20_nt16.b14", "resnet20_nt16.b14r51", "suite/HarrisCornerDetection",
            "suite/LinearRegression", "suite/MLP", "suite/Multivariate", "suite/PolynomialRegression", "suite/SobelFilter"]
# the headline program: (groups, hops absorbed, members, distinct member offsets, of them composite) per f.  Its maximal chains are
# 4 x 128, 5 x 112, 6 x 80, 3 x 1, 2 x 7, 1 x 12 (length x count): at f = 6 every chain of two or more hops is one group, 128 + 112 + 80 + 1 + 7.
HEADLINE = {2: (728, 1456, 2184, 16, 5), 3: (648, 1569, 3036, 28, 16), 6: (328, 1569, 10460, 94, 82)}


@pytest.mark.parametrize("f", [2, 3, 6])
@pytest.mark.parametrize("name", FIXTURES)
def test_groups_of_the_committed_programs(driver, tmp_path, name, f):
    raw = gzip.decompress((GOLDEN / (name + ".hevm.gz")).read_bytes())
    slots = json.loads((GOLDEN / (name + ".json")).read_text())["slots"]
    path = tmp_path / "p.hevm"
    path.write_bytes(raw)
    prog = ha.unpack_hevm(raw)
    rotates, groups = groups_of(driver, path, f, slots)
    assert rotates == sum(1 for op in prog["ops"] if int(op[0]) == ROT)
    want = flatten_groups(prog["ops"], prog["res_dst"], f, slots)
    assert groups == want
    for closing, _, pairs, members in groups:  # what the driver names is what it says
        assert 2 <= len(pairs) <= f and len(members) == (1 << len(pairs)) - 1 and pairs[-1][1] == closing
        assert all(int(prog["ops"][r][0]) == ROT and int(prog["ops"][a][0]) == ADDCC and r < a for r, a in pairs)
    if name == "resnet20":
        assert totals(groups) == HEADLINE[f]
        assert sorted(len(g[2]) for g in groups if f == 6) == ([2] * 7 + [3] + [4] * 128 + [5] * 112 + [6] * 80 if f == 6 else [])


def naf_hops(offset):
    """key switches of one rotate instruction under the default key set (+-2^k): the non-zero digits of the offset's non-adjacent form"""
    v, n = abs(offset), 0
    while v:
        z = (2 - (v & 3)) if v & 1 else 0
        v, n = (v - z) >> 1, n + (1 if z else 0)
    return n


def ks_depth(ops, groups):
    """ASAP depth of the program counting one per key-switch sequence and one per opcode 10, with `groups` applied: a group is one
    sequence that reads the stage's source; the stage's rotations and other adds are gone"""
    closing = {g[0]: g[1] for g in groups}
    gone = {i for g in groups for pair in g[2] for i in pair} - set(closing)
    cur, d = {}, {}
    for i, (opc, dst, lhs, rhs) in enumerate([tuple(int(x) for x in op) for op in ops]):
        if (opc not in UNARY and opc not in BINARY) or (opc == MODSWITCH and s16(rhs) <= 0) or (opc == ROT and s16(rhs) == 0 and dst == lhs):
            continue
        if i in closing:
            d[i] = (d[closing[i]] if closing[i] >= 0 else 0) + 1
        elif i not in gone:
            srcs = [cur.get(lhs)] + ([cur.get(rhs)] if opc in BINARY else [])
            cost = naf_hops(s16(rhs)) if opc == ROT else 1 if opc in (MULCC, BOOT, 17, 20) else 0
            d[i] = max([d[v] for v in srcs if v is not None] + [0]) + cost
        cur[dst] = i
    return max(d.values())


@pytest.mark.parametrize("name,before,after", [("resnet20", 564, 483), ("resnet20.b13", 474, 393), ("resnet20_nt16.b14", 480, 368)])
def test_key_switch_depth_with_every_chain_flattened_whole(driver, tmp_path, name, before, after):
    """the dependent key-switch sequences of a run, from the pass's own groups at f = 6 (the restatement's are the same groups, above)"""
    raw = gzip.decompress((GOLDEN / (name + ".hevm.gz")).read_bytes())
    slots = json.loads((GOLDEN / (name + ".json")).read_text())["slots"]
    path = tmp_path / "p.hevm"
    path.write_bytes(raw)
    ops = ha.unpack_hevm(raw)["ops"]
    assert ks_depth(ops, []) == before
    assert ks_depth(ops, groups_of(driver, path, 6, slots)[1]) == after


def program(tmp_path, ops, args=4, level=5, results=()):
    """ops over registers: 0 .. args - 1 are the inputs at `level` primes; results: the registers the program returns"""
    raw = ha.pack_hevm([40] * args, [level] * args, [40] * len(results), [level] * len(results), list(results), 64, 0, level, ops)
    path = tmp_path / "hand.hevm"
    path.write_bytes(raw)
    return path


def chain(offsets, first_reg=10, src=0, swap=()):
    """y' = y + rotate(y, o) per offset: instruction 2k rotates, 2k + 1 adds (hops in `swap`: rotate first in the add) -> (ops, last register)"""
    ops, y, reg = [], src, first_reg
    for k, o in enumerate(offsets):
        ops.append((ROT, reg, y, o & 0xFFFF))
        ops.append((ADDCC, reg + 1, reg, y) if k in swap else (ADDCC, reg + 1, y, reg))
        y, reg = reg + 1, reg + 2
    return ops, y


def both(driver, tmp_path, ops, results, f, slots=2048, keyed=None):
    """the driver's groups, which must be the restatement's"""
    got = groups_of(driver, program(tmp_path, ops, results=results), f, slots, keyed)[1]
    assert got == flatten_groups(ops, list(results), f, slots, keyed)
    return got


def test_a_chain_in_either_operand_order(driver, tmp_path):
    ops, y = chain([1, 2, 4], swap=(1,))
    got = both(driver, tmp_path, ops, [y], 6)
    assert got == [(5, -1, [(0, 1), (2, 3), (4, 5)], [1, 2, 3, 4, 5, 6, 7])]
    # negative offsets and sums that wrap around the slot count
    ops, y = chain([-1, 1024, 1000], src=2)
    assert both(driver, tmp_path, ops, [y], 3) == [(5, -3, [(0, 1), (2, 3), (4, 5)], [-1, 1024, 1023, 1000, 999, -24, -25])]


def test_seven_hops_at_three_are_three_two_two(driver, tmp_path):
    ops, y = chain([1, 2, 4, 8, 16, 32, 64])
    got = both(driver, tmp_path, ops, [y], 3)
    assert [(g[0], g[1], len(g[2])) for g in got] == [(5, -1, 3), (9, 5, 2), (13, 9, 2)]
    assert got[1][3] == [8, 16, 24] and got[2][3] == [32, 64, 96]
    assert [len(g[2]) for g in both(driver, tmp_path, ops, [y], 6)] == [4, 3]
    assert [len(g[2]) for g in both(driver, tmp_path, ops, [y], 2)] == [2, 2, 2]  # 2 + 2 + 2 + 1: the last hop stays as written


def test_an_interior_value_with_a_third_reader_cuts_the_chain(driver, tmp_path):
    ops, y = chain([1, 2, 4, 8])
    ops.append((MULCC, 30, 13, 13))  # y_2 (register 13, instruction 3) has readers beyond its hop
    got = both(driver, tmp_path, ops, [y, 30], 6)
    assert [(g[0], g[1], [p[1] for p in g[2]]) for g in got] == [(3, -1, [1, 3]), (7, 3, [5, 7])]


def test_an_interior_value_that_is_a_result_cuts_the_chain(driver, tmp_path):
    ops, y = chain([1, 2, 4, 8, 16])
    got = both(driver, tmp_path, ops, [y, 15], 6)  # register 15 = y_3 (instruction 5)
    assert [(g[0], g[1], len(g[2])) for g in got] == [(5, -1, 3), (9, 5, 2)]
    # a register that merely still names an interior value, without being a result, does not
    assert [len(g[2]) for g in both(driver, tmp_path, ops, [y], 6)] == [5]


def test_a_rotation_read_twice_is_no_hop(driver, tmp_path):
    ops, y = chain([1, 2, 4, 8, 16])
    ops.append((ADDCC, 31, 14, 1))  # the third hop's rotation (register 14) has a second reader
    got = both(driver, tmp_path, ops, [y, 31], 6)
    assert [(g[0], g[1], [p[1] for p in g[2]]) for g in got] == [(3, -1, [1, 3]), (9, 5, [7, 9])]
    # ... nor is a rotation that is a result, nor a rotation of another value than the add's other operand
    ops, y = chain([1, 2, 4])
    assert [len(g[2]) for g in both(driver, tmp_path, ops, [y, 12], 6)] == []
    ops = [(ROT, 10, 0, 1), (ADDCC, 11, 1, 10), (ROT, 12, 11, 2), (ADDCC, 13, 11, 12), (ROT, 14, 13, 4), (ADDCC, 15, 13, 14)]
    assert [(g[0], len(g[2])) for g in both(driver, tmp_path, ops, [15], 6)] == [(5, 2)]


def test_a_subset_sum_of_zero_leaves_the_stage_as_written(driver, tmp_path):
    """slots = 2048: 1024 + 1024 = 0, so would 3 + 5 - 8; two subset sums that coincide (1 + 2 = 3) stay two members"""
    ops, y = chain([1024, 1024])
    assert both(driver, tmp_path, ops, [y], 2) == []
    ops, y = chain([3, 5, -8, 16])
    assert [(g[0], len(g[2])) for g in both(driver, tmp_path, ops, [y], 6)] == []
    assert [(g[0], len(g[2])) for g in both(driver, tmp_path, ops, [y], 2)] == [(3, 2), (7, 2)]
    assert [(g[0], len(g[2])) for g in both(driver, tmp_path, ops, [y], 3)] == [(3, 2), (7, 2)]
    ops, y = chain([1, 2, 3])
    assert both(driver, tmp_path, ops, [y], 3)[0][3] == [1, 2, 3, 3, 4, 5, 6]


def test_a_missing_key_in_the_middle_of_a_chain(driver, tmp_path):
    """6 hops at f = 2: stages (1, 2), (4, 8), (16, 32); without a key for 4 + 8 the middle stage runs as the program's hops"""
    ops, y = chain([1, 2, 4, 8, 16, 32])
    keyed = {1, 2, 3, 4, 8, 16, 32, 48}
    assert [(g[0], g[3]) for g in both(driver, tmp_path, ops, [y], 2, keyed=keyed)] == [(3, [1, 2, 3]), (11, [16, 32, 48])]
    assert [g[0] for g in both(driver, tmp_path, ops, [y], 2, keyed=keyed | {12})] == [3, 7, 11]
    assert both(driver, tmp_path, ops, [y], 6, keyed=keyed | {12}) == []
    # keys are looked up modulo the slot count
    assert [g[0] for g in both(driver, tmp_path, ops, [y], 2, slots=2048, keyed={1, 2, 3 - 2048})] == [3]


def test_the_driver_refuses_what_it_cannot_run(driver, tmp_path):
    ops, y = chain([1, 2])
    path = program(tmp_path, ops, results=[y])
    for args in (["1", "2048"], ["7", "2048"], ["2", "1000"]):
        r = subprocess.run([str(driver), "flatten", str(path)] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "F is 2 .. 6" in r.stderr
