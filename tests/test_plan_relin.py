"""The grouping pass of lazy relinearisation (dacapo_amd/csrc/plan_relin.cpp) on its own, without a GPU.

`make -C dacapo_amd/csrc plan_groups_asan` builds the pass -- host-only C++, plain arrays in, groups out --, the library's walk of a program
(plan_flow.cpp) and a small driver (plan_groups_main.cpp) under AddressSanitizer + UBSan.  `plan_groups_asan relin` reads a .hevm program,
walks it as the library does and prints the groups: maximal trees of addcc / negate
over single-use mulcc results at one level, which one key switch can relinearise (dc_ct_mul_sum_relin).

  * the committed programs: suite/Multivariate has three groups of three products, HarrisCornerDetection and SobelFilter one group of two,
    MLP, PolynomialRegression, LinearRegression, resnet20 and resnet20_nt16.b14 none;
  * hand-made op lists: a product with two readers, a product that is a result, nested negates (the signs), a tree with a bare ciphertext
    leaf (cut down to its qualifying subtree), leaves at two levels, a tree above the cap;
  * the sanitizers stay silent (-fno-sanitize-recover: a finding is a non-zero exit status and text on stderr)."""
import gzip
import shutil
import subprocess
from pathlib import Path

import pytest

from dacapo_amd import hevm_asm as ha

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dacapo_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden"
DRIVER = CSRC / "build_asan" / "plan_groups_asan"

ROT, NEG, RESCALE, MODSWITCH, ADDCC, MULCC = 1, 2, 3, 4, 6, 8


@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no g++ / make")
    r = subprocess.run(["make", "-C", str(CSRC), "plan_groups_asan"], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()) and "error:" not in r.stderr:
        pytest.skip("this toolchain has no AddressSanitizer runtime: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-2000:]
    return DRIVER


def groups_of(driver, hevm_path, cap=None):
    """[(closing op, level, [(mul op, sign), ...]), ...] as the driver prints them; stderr must be empty"""
    r = subprocess.run([str(driver), "relin", str(hevm_path)] + ([str(cap)] if cap is not None else []), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    head = lines[0].split()
    assert head[0] == "products" and head[2] == "groups" and head[4] == "saved"
    out = []
    for line in lines[1:]:
        left, right = line.split(":")
        w = left.split()
        assert w[0] == "group" and w[1] == "closing" and w[3] == "level"
        out.append((int(w[2]), int(w[4]), [(int(m[1:]), 1 if m[0] == "+" else -1) for m in right.split()]))
    assert int(head[3]) == len(out) and int(head[5]) == sum(len(g[2]) - 1 for g in out)
    return int(head[1]), out


@pytest.mark.parametrize("name,products,sizes", [("suite/Multivariate", 27, [3, 3, 3]), ("suite/HarrisCornerDetection", 6, [2]),
                                                 ("suite/SobelFilter", 5, [2]), ("suite/MLP", 1, []), ("suite/PolynomialRegression", 10, []),
                                                 ("suite/LinearRegression", 3, []), ("resnet20", 361, []), ("resnet20_nt16.b14", 361, [])])
def test_groups_of_the_committed_programs(driver, tmp_path, name, products, sizes):
    raw = gzip.decompress((GOLDEN / (name + ".hevm.gz")).read_bytes())
    path = tmp_path / "p.hevm"
    path.write_bytes(raw)
    n, groups = groups_of(driver, path)
    assert n == products
    assert [len(g[2]) for g in groups] == sizes
    ops = ha.unpack_hevm(raw)["ops"]
    for closing, _, members in groups:  # what the driver names is what it says: products below an addcc / negate, all before it
        assert int(ops[closing][0]) in (ADDCC, NEG)
        assert all(int(ops[m][0]) == MULCC and m < closing for m, _ in members)


def program(tmp_path, ops, args=4, level=5, results=()):
    """ops over registers: 0 .. args - 1 are the inputs at `level` primes; results: the registers the program returns"""
    raw = ha.pack_hevm([40] * args, [level] * args, [40] * len(results), [level] * len(results), list(results), 64, 0, level, ops)
    path = tmp_path / "hand.hevm"
    path.write_bytes(raw)
    return path


def test_a_sum_of_two_products_with_nested_negates(driver, tmp_path):
    """r = -(-(x y) + -(-(z w))) + (u u)  ->  + x y, - z w, + u u: a leaf's sign is the parity of the negates above it"""
    ops = [(MULCC, 10, 0, 1),   # 0: x y
           (NEG, 11, 10, 0),    # 1
           (MULCC, 12, 2, 3),   # 2: z w
           (NEG, 13, 12, 0),    # 3
           (NEG, 14, 13, 0),    # 4
           (ADDCC, 15, 11, 14), # 5: -(x y) + (z w)
           (NEG, 16, 15, 0),    # 6: (x y) - (z w)
           (MULCC, 17, 0, 0),   # 7: x x
           (ADDCC, 18, 16, 17)] # 8
    n, groups = groups_of(driver, program(tmp_path, ops, results=[18]))
    assert n == 3 and groups == [(8, 5, [(0, 1), (2, -1), (7, 1)])]


def test_a_product_with_two_readers_stays_a_mulcc(driver, tmp_path):
    """x y feeds the sum AND a rotation: it is materialised anyway; the other two products still form a group.  p + p reads p twice."""
    ops = [(MULCC, 10, 0, 1), (MULCC, 11, 2, 3), (MULCC, 12, 1, 2),
           (ADDCC, 13, 11, 12),  # 3: group of two
           (ADDCC, 14, 13, 10),  # 4: ... + x y, which op 5 reads as well
           (ROT, 15, 10, 1),
           (MULCC, 16, 0, 3),
           (ADDCC, 17, 16, 16)]  # 7: p + p
    n, groups = groups_of(driver, program(tmp_path, ops, results=[14, 15, 17]))
    assert n == 4 and groups == [(3, 5, [(1, 1), (2, 1)])]


def test_a_rotation_by_zero_onto_its_own_register_changes_nothing(driver, tmp_path):
    """p = x y; rotate p by 0 onto its own register; q = z w; p + q: the rotation leaves the register's value alone (the plan adds no hop), so
    the two products are one group.  By 0 into ANOTHER register it is a copy, a reader of p: no group."""
    ops = [(MULCC, 10, 0, 1), (ROT, 10, 10, 0), (MULCC, 11, 2, 3), (ADDCC, 12, 10, 11)]
    assert groups_of(driver, program(tmp_path, ops, results=[12])) == (2, [(3, 5, [(0, 1), (2, 1)])])
    ops = [(MULCC, 10, 0, 1), (ROT, 13, 10, 0), (MULCC, 11, 2, 3), (ADDCC, 12, 13, 11)]
    assert groups_of(driver, program(tmp_path, ops, results=[12])) == (2, [])


def test_a_product_that_is_a_result_stays_a_mulcc(driver, tmp_path):
    ops = [(MULCC, 10, 0, 1), (MULCC, 11, 2, 3), (ADDCC, 12, 10, 11)]
    assert groups_of(driver, program(tmp_path, ops, results=[12]))[1] == [(2, 5, [(0, 1), (1, 1)])]
    assert groups_of(driver, program(tmp_path, ops, results=[12, 11]))[1] == []
    # an interior node that is a result cuts the tree there: the inner sum is a group, the outer add an ordinary addcc
    ops += [(MULCC, 13, 0, 2), (ADDCC, 14, 12, 13)]
    assert groups_of(driver, program(tmp_path, ops, results=[14]))[1] == [(4, 5, [(0, 1), (1, 1), (3, 1)])]
    assert groups_of(driver, program(tmp_path, ops, results=[14, 12]))[1] == [(2, 5, [(0, 1), (1, 1)])]


def test_a_mixed_tree_is_cut_to_its_qualifying_subtrees(driver, tmp_path):
    """((x y - z w) + c) + (u u + v v) with c a bare ciphertext: the two inner sums are groups, the adds above them are not"""
    ops = [(MULCC, 10, 0, 1), (MULCC, 11, 2, 3), (NEG, 12, 11, 0),
           (ADDCC, 13, 10, 12),  # 3: x y - z w
           (ADDCC, 14, 13, 2),   # 4: + c
           (MULCC, 15, 0, 0), (MULCC, 16, 1, 1),
           (ADDCC, 17, 15, 16),  # 7
           (ADDCC, 18, 14, 17)]  # 8
    assert groups_of(driver, program(tmp_path, ops, results=[18]))[1] == [(3, 5, [(0, 1), (1, -1)]), (7, 5, [(5, 1), (6, 1)])]


def test_leaves_at_two_levels_do_not_join(driver, tmp_path):
    """x y at 5 primes and (x' y') at 4 (operands mod-switched down): the add above them is no interior node.  With a third product at 4
    primes the lower two form the group."""
    ops = [(MULCC, 10, 0, 1),
           (MODSWITCH, 11, 0, 1), (MODSWITCH, 12, 1, 1),
           (MULCC, 13, 11, 12),
           (ADDCC, 14, 10, 13)]
    assert groups_of(driver, program(tmp_path, ops, results=[14]))[1] == []
    ops = ops[:4] + [(MULCC, 15, 11, 11), (ADDCC, 16, 13, 15), (ADDCC, 17, 10, 16)]
    assert groups_of(driver, program(tmp_path, ops, results=[17]))[1] == [(5, 4, [(3, 1), (4, 1)])]


def test_a_tree_above_the_cap_is_split(driver, tmp_path):
    """a chain of 6 products under cap 4: the chain's first four form the group, the adds above take the last two as ordinary mulcc; a
    balanced tree of 3 + 3 under cap 4 is two groups of three"""
    ops, acc = [(MULCC, 10, 0, 1)], 10
    for k in range(1, 6):
        ops.append((MULCC, 10 + 2 * k, k % 4, (k + 1) % 4))
        ops.append((ADDCC, 11 + 2 * k, acc, 10 + 2 * k))
        acc = 11 + 2 * k
    path = program(tmp_path, ops, results=[acc])
    assert [len(g[2]) for g in groups_of(driver, path)[1]] == [6]
    assert groups_of(driver, path, cap=4)[1] == [(6, 5, [(0, 1), (1, 1), (3, 1), (5, 1)])]

    def three(regs):
        return [(MULCC, regs, 0, 1), (MULCC, regs + 1, 1, 2), (ADDCC, regs + 2, regs, regs + 1), (MULCC, regs + 3, 2, 3), (ADDCC, regs + 4, regs + 2, regs + 3)]

    ops = three(10) + three(20) + [(ADDCC, 30, 14, 24)]
    path = program(tmp_path, ops, results=[30])
    assert [len(g[2]) for g in groups_of(driver, path)[1]] == [6]
    assert groups_of(driver, path, cap=4)[1] == [(4, 5, [(0, 1), (1, 1), (3, 1)]), (9, 5, [(5, 1), (6, 1), (8, 1)])]
    r = subprocess.run([str(driver), "relin", str(path), "1"], capture_output=True, text=True)
    assert r.returncode == 2 and "at least 2" in r.stderr
