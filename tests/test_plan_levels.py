"""The plan's slack-aware levelling pass (dacapo_amd/csrc/plan_levels.cpp, option plan_level = 1) on its own, without a GPU.

`make -C dacapo_amd/csrc plan_levels_asan` builds the pass -- host-only C++, plain arrays in, waves out -- with a small driver
(plan_levels_main.cpp) under AddressSanitizer + UBSan.  The driver reads DAGs from a text file and prints the waves; everything asserted here
is recomputed in Python from those waves alone (ASAP and ALAP waves, buckets, step counts), never taken from the pass's own statistics:

  * every consumer's wave is later than every producer's, every operation stays inside its window [ASAP, ALAP], the depth does not grow;
  * an operation marked fixed (a P_ROTSUM group) keeps its wave;
  * an operation that moved to join a step joined a NON-EMPTY bucket of its exact key (kind, level, target), and its arrival did not make
    that bucket spill into another max_batch chunk;
  * the plan never has more steps than the ASAP plan, and strictly fewer on the hand-written DAG where ASAP leaves a multiply, a rescale and
    an opcode 10 alone in a wave while their windows each contain a wave with a step of their key;
  * plan_level = 0 returns the ASAP waves unchanged."""
import shutil
import subprocess
from collections import defaultdict
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "dacapo_amd" / "csrc"
DRIVER = CSRC / "build_asan" / "plan_levels_asan"

ROT, MULCC, RESCALE, SUM, NEG, MULP, ADDP, BOOT, ROTSUM = 0, 1, 2, 3, 4, 5, 6, 8, 10
HEAVY = {ROT, MULCC, RESCALE, BOOT, ROTSUM}
LAUNCHES = {ROT: 5, MULCC: 5, ROTSUM: 5, RESCALE: 3, BOOT: 4}
STAYED, JOINED, FORCED = 0, 1, 2


@pytest.fixture(scope="module")
def driver():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no g++ / make")
    r = subprocess.run(["make", "-C", str(CSRC), "plan_levels_asan"], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "sanitize" in r.stderr.lower()) and "error:" not in r.stderr:
        pytest.skip("this toolchain has no AddressSanitizer runtime: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-2000:]
    return DRIVER


def op(kind, level, prods=(), target=0, cap=None, fixed=0, link_prev=-1):
    return {"kind": kind, "level": level, "target": target, "cap": cap if cap is not None else (4 if kind in HEAVY else 4096), "fixed": fixed,
            "launches": LAUNCHES.get(kind, 1), "link_prev": link_prev, "prods": list(prods)}


def asap_of(dag):
    w = []
    for o in dag:
        w.append(1 + max((w[p] for p in o["prods"]), default=0))
    return w


def alap_of(dag, depth):
    a, asap = [depth] * len(dag), asap_of(dag)
    for i in range(len(dag) - 1, -1, -1):
        if dag[i]["fixed"]:  # (it keeps its wave, so its producers must be done before it)
            a[i] = asap[i]
        for p in dag[i]["prods"]:
            a[p] = min(a[p], a[i] - 1)
    return a


def key(o):
    return (o["kind"], o["level"], o["target"])


def steps_of(dag, wave):
    b, cap = defaultdict(int), {}
    for o, w in zip(dag, wave):
        b[(w, key(o))] += 1
        cap[key(o)] = o["cap"]
    return sum(-(-n // cap[k]) for (w, k), n in b.items())


def run_driver(driver, tmp_path, dags, mode):
    lines = [str(len(dags))]
    for dag in dags:
        asap = asap_of(dag)
        lines.append(f"{len(dag)} {mode}")
        for o, a in zip(dag, asap):
            lines.append(" ".join(str(v) for v in [o["kind"], o["level"], o["target"], o["cap"], o["fixed"], o["launches"], o["link_prev"], a,
                                                    len(o["prods"])] + o["prods"]))
    f = tmp_path / f"dags{mode}.txt"
    f.write_text("\n".join(lines) + "\n")
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    r = subprocess.run([str(driver), str(f)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-300:], r.stderr[-2000:])
    out = r.stdout.strip().splitlines()
    assert len(out) == 3 * len(dags)
    res = []
    for d in range(len(dags)):
        head = out[3 * d].split()
        stats = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
        wave = [int(v) for v in out[3 * d + 1].split()[1:]]
        how = [int(v) for v in out[3 * d + 2].split()[1:]]
        assert len(wave) == len(dags[d]) == len(how)
        res.append((stats, wave, how))
    return res


def random_dag(seed):
    """mixed kinds and levels, a long chain (so that the rest has slack) with side branches of every kind hanging off it and off each other"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(30, 140))
    kinds = [ROT, MULCC, RESCALE, SUM, NEG, MULP, ADDP, BOOT, ROTSUM]
    weights = np.array([3, 4, 4, 3, 1, 1, 1, 3, 0.3])
    dag = []
    chain_tip = -1
    for i in range(n):
        kind = int(rng.choice(kinds, p=weights / weights.sum()))
        level = int(rng.integers(1, 4))
        prods = []
        if i:
            if rng.random() < 0.45 and chain_tip >= 0:
                prods.append(chain_tip)        # extends the long chain
            elif rng.random() < 0.8:
                prods.append(int(rng.integers(max(0, i - 12), i)))
            if kind in (MULCC, SUM) and rng.random() < 0.6:
                prods.append(int(rng.integers(0, i)))
        if prods and prods[0] == chain_tip or chain_tip < 0:
            chain_tip = i
        prods = sorted(set(prods))
        link_prev = -1
        if kind in (RESCALE, BOOT, MULCC) and prods and rng.random() < 0.7:  # (the pass takes any earlier operation as a hand-off producer)
            link_prev = prods[0]
        cap = int(rng.choice([1, 2, 4, 64])) if kind in HEAVY else 4096
        dag.append(op(kind, level, prods, target=3 if kind == BOOT else (-1 if kind == ROT and rng.random() < 0.1 else 0), cap=cap,
                      fixed=int(kind == ROTSUM), link_prev=link_prev))
    # one capacity per bucket key, as in the plan (a step's chunk depends on its kind alone)
    cap_of = {}
    for o in dag:
        o["cap"] = cap_of.setdefault(key(o)[0], o["cap"])
    return dag


def hand_written_dag():
    """a critical chain of three (multiply -> rescale -> opcode 10) rounds, waves 1 .. 9, and a side chain rotation -> multiply -> rescale ->
    opcode 10 that joins it by a sum in wave 10.  ASAP runs the side multiply in wave 2 (beside a rescale), its rescale in wave 3 (beside an
    opcode 10) and its opcode 10 in wave 4 (beside a multiply): three one-item steps of their own, although waves 4, 5 and 6 hold a step of
    each one's key and lie inside their windows [2, 7], [3, 8], [4, 9]."""
    dag = []
    prev = -1
    for _ in range(3):
        dag.append(op(MULCC, 3, [prev] if prev >= 0 else []))
        dag.append(op(RESCALE, 3, [len(dag) - 1], link_prev=len(dag) - 1))
        dag.append(op(BOOT, 2, [len(dag) - 1], target=3, link_prev=len(dag) - 1))
        prev = len(dag) - 1
    dag.append(op(ROT, 3))
    dag.append(op(MULCC, 3, [len(dag) - 1]))
    dag.append(op(RESCALE, 3, [len(dag) - 1], link_prev=len(dag) - 1))
    dag.append(op(BOOT, 2, [len(dag) - 1], target=3, link_prev=len(dag) - 1))
    dag.append(op(SUM, 3, [prev, len(dag) - 1]))
    return dag


def check_invariants(dag, wave, how):
    asap = asap_of(dag)
    depth = max(asap)
    alap = alap_of(dag, depth)
    assert max(wave) <= depth
    for i, o in enumerate(dag):
        assert asap[i] <= wave[i] <= alap[i], (i, asap[i], wave[i], alap[i])
        for p in o["prods"]:
            assert wave[p] < wave[i], (i, p)
        if o["fixed"] or asap[i] == alap[i]:
            assert wave[i] == asap[i] and how[i] == STAYED, i
        assert (how[i] == STAYED) == (wave[i] == asap[i]), i
    # replay the arrivals: the operations without slack seed the buckets, the others arrive in program order
    count = defaultdict(int)
    for i, o in enumerate(dag):
        if o["fixed"] or asap[i] == alap[i]:
            count[(wave[i], key(o))] += 1
    for i, o in enumerate(dag):
        if o["fixed"] or asap[i] == alap[i]:
            continue
        b = (wave[i], key(o))
        if how[i] == JOINED:  # a bucket of its exact key that holds a step already, and room in that step's last chunk
            assert count[b] > 0 and count[b] % o["cap"] != 0, (i, b, count[b])
        count[b] += 1
    assert steps_of(dag, wave) <= steps_of(dag, asap)


def test_plan_level_0_returns_the_asap_waves(driver, tmp_path):
    dags = [random_dag(s) for s in range(20)] + [hand_written_dag()]
    for dag, (stats, wave, how) in zip(dags, run_driver(driver, tmp_path, dags, 0)):
        assert wave == asap_of(dag) and stats["moved"] == 0 and not any(how)
        assert stats["steps"] == steps_of(dag, wave) and stats["waves"] == max(wave)


def test_random_dags_keep_every_invariant_and_never_gain_steps(driver, tmp_path):
    dags = [random_dag(s) for s in range(300)]
    moved = fewer = 0
    for dag, (stats, wave, how) in zip(dags, run_driver(driver, tmp_path, dags, 1)):
        check_invariants(dag, wave, how)
        assert stats["steps"] == steps_of(dag, wave)  # (the pass's own count agrees with the one recomputed here)
        moved += stats["moved"] > 0
        fewer += steps_of(dag, wave) < steps_of(dag, asap_of(dag))
    assert moved > 100 and fewer > 100, (moved, fewer)  # (the DAGs do have slack: the pass is exercised, not idle)


def test_hand_written_dag_loses_the_three_lonely_steps_and_keeps_its_links(driver, tmp_path):
    dag = hand_written_dag()
    (s0, w0, _), = run_driver(driver, tmp_path, [dag], 0)
    (s1, w1, how), = run_driver(driver, tmp_path, [dag], 1)
    check_invariants(dag, w1, how)
    assert w0[10:13] == [2, 3, 4] and w1[10:13] == [4, 5, 6] and how[10:13] == [JOINED] * 3
    assert steps_of(dag, w0) == 14 and steps_of(dag, w1) == 11 and s1["steps"] == 11
    assert s1["waves"] == s0["waves"] == 10
    # the side chain moved as a whole: its rescale and its opcode 10 sit in the steps that consume their producers' step-mates, so the
    # links multiply -> rescale -> opcode 10 of the second round still match item for item (two items each now)
    assert s0["links"] == 8 and s1["links"] == 6 and s1["launches"] < s0["launches"]
