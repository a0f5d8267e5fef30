"""The synthetic edge cases of tests/synth.py (lin_cases, orbit_cases) without a device: the generators still produce the
inputs the goldens were made from (SHA-256), the literal oracles recompute the goldens' quick cases, and the HOST engines
(plo_inplace.hpp through `bin/inplacer --gpu 0 --costs`, plo_orbit.hpp through `bin/orbiter --gpu 0 --costs`) give the
goldens' counts on every case -- the cases the device refuses included, which the oracle scores here."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import lin_oracle
import orbit_oracle
import synth
from plo_testlib import GOLDEN, ROOT

INP = os.path.join(ROOT, "bin", "inplacer")
ORB = os.path.join(ROOT, "bin", "orbiter")
LIN_GOLD = json.load(open(os.path.join(GOLDEN, "lin_synth_costs.json")))
ORB_GOLD = json.load(open(os.path.join(GOLDEN, "orbit_synth_costs.json")))
LIN_CASES = {c.name: c for c in synth.lin_cases()}
ORB_CASES = {c.name: c for c in synth.orbit_cases()}
LIN_TIE = {c.name: c for c in synth.lin_tie_cases()}
ORB_TIE = {c.name: c for c in synth.orbit_tie_cases()}
# what the tools' command lines cannot express (at most 5 per tool)
INPLACER_SKIPS = []
ORBITER_SKIPS = ["orbit_refuse_mod2p31"]           # -m strips the factors 2 of a modulus (src/orbiter.cpp:421-422): 2^31 becomes 2
REFUSAL_SEEDS = [synth.BASE_SEED, 0, 1, 2]


def run(cmd, stdin=None):
    r = subprocess.run(cmd, input=stdin, capture_output=True, text=True, timeout=300)
    return r.returncode, r.stdout, r.stderr


def runs_of(seeds):
    """the (seed0, n) runs of --costs that cover `seeds` (BASE_SEED is the first line of every run)"""
    rest = sorted(s for s in seeds if s != synth.BASE_SEED)
    runs = []
    for s in rest:
        if runs and runs[-1][0] + runs[-1][1] == s:
            runs[-1][1] += 1
        else:
            runs.append([s, 1])
    return runs or [[0, 0]]


def test_generators_reproduce_the_goldens_inputs():
    for gold, cases, ties in ((LIN_GOLD, LIN_CASES, LIN_TIE), (ORB_GOLD, ORB_CASES, ORB_TIE)):
        assert [e["name"] for e in gold["cases"]] == list(cases)
        for e in gold["cases"]:
            c = cases[e["name"]]
            assert c.sha256 == e["sha256"] and c.family == e["family"], e["name"]
            assert e.get("refusal") == c.refusal, e["name"]
            if not c.refusal:
                assert (e["mode"], e["seeds"], e["quick"]) == (c.mode, c.seeds, c.quick), e["name"]
                assert set(synth.SEEDS_LIST) == set(e["seeds"]) and len(e["out"]) == len(e["seeds"])
        assert [t["name"] for t in gold["tie"]] == list(ties)
        for t in gold["tie"]:
            assert ties[t["name"]].sha256 == t["sha256"], t["name"]
        modes = [e["mode"] for e in gold["cases"] if "mode" in e]
        assert abs(modes.count("list") - modes.count("runs")) <= 2
    assert len(LIN_CASES) >= 55 and len(ORB_CASES) >= 45


def test_generated_cases_are_what_the_issue_names():
    """the edges by name: a failure of a family names its edge"""
    fam = lambda cases, f: [c for c in cases.values() if c.family == f]  # noqa: E731
    assert sorted(c.m for c in fam(LIN_CASES, "a") if c.unit) == [1, 2, 63, 64, 65, 128, 129]
    assert all(any(not any(i == r for (r, _) in c.ent) for i in range(c.m)) for c in fam(LIN_CASES, "b"))
    lens = lambda c: sorted(sum(1 for (r, _) in c.ent if r == i) for i in range(c.m))  # noqa: E731
    assert any(lens(c)[-1] == 64 and 63 in lens(c) and lens(c)[0] == 1 for c in fam(LIN_CASES, "c")) and all(lens(c)[-1] <= 64 and c.nnz < 400 for c in fam(LIN_CASES, "c"))
    assert sorted({c.n for c in fam(LIN_CASES, "d")}) == [300, 8193, 16382] and all({c.n - 1, c.n - 2} <= {j for (_, j) in c.ent} for c in fam(LIN_CASES, "d"))
    assert all(c.waves == 1 for f in "ghi" for c in fam(LIN_CASES, f)) and all(c.waves == 4 for f in "abcdef" for c in fam(LIN_CASES, f))
    assert {c.mkn for c in fam(ORB_CASES, "a")} == {c.mkn for c in fam(ORB_CASES, "e")} == {mkn for mkn, _ in synth.A_SHAPES}
    assert {c.r for c in fam(ORB_CASES, "a")} == {1, 2, 33, 64, 65}
    assert sorted(c.waves for c in fam(ORB_CASES, "b") if c.measure == synth.DENSITY) == [1, 2, 4]
    assert {c.modulus for c in fam(ORB_CASES, "c")} == {0, 3, 5, 9, 15, 131071, 2147483629, 2147483647, 2147483645}
    assert all(c.dev_nnz < c.nnz for c in fam(ORB_CASES, "c") if c.modulus)
    assert all(c.modulus == 131071 and c.measure == synth.CANONICAL for c in fam(ORB_CASES, "f")) and len(fam(ORB_CASES, "f")) == 2


def test_lin_oracle_recomputes_the_quick_cases():
    quick = [e for e in LIN_GOLD["cases"] if e.get("quick")]
    assert len(quick) >= 45 and max(LIN_CASES[e["name"]].m for e in quick) == 129 and any(LIN_CASES[e["name"]].family == "c" for e in quick)
    for e in quick:
        c = LIN_CASES[e["name"]]
        rows = lin_oracle.rows_of(c.m, c.n, c.ent)
        assert [lin_oracle.cost6(rows, c.n, s) for s in e["seeds"]] == e["out"], e["name"]


def orbit_mats(c):
    mats = [orbit_oracle.dense(*M) for M in (c.L, c.R, c.P)]
    return [M if orbit_oracle.small_ints(M) is None else orbit_oracle.small_ints(M) for M in mats]


def test_orbit_oracle_recomputes_the_quick_cases():
    quick = [e for e in ORB_GOLD["cases"] if e.get("quick")]
    assert len(quick) >= 25 and max(max(ORB_CASES[e["name"]].mkn) for e in quick) == 16 and any(min(ORB_CASES[e["name"]].mkn) == 9 for e in quick)
    for e in quick:
        c = ORB_CASES[e["name"]]
        mats = orbit_mats(c)
        assert [list(orbit_oracle.cost3(mats, c.mkn, s, modulus=c.modulus, measure=c.measure)) for s in e["seeds"]] == e["out"], e["name"]


def test_tie_blocks_tie():
    """the searches' cases do tie: the minimum of each block is reached by more than one candidate"""
    for t in LIN_GOLD["tie"]:
        o = t["out"]
        keys = [(o[6 * k + 3 * v], o[6 * k + 3 * v + 1]) for k in range(t["n"]) for v in (0, 1)]
        assert len(o) == 6 * t["n"] and keys.count(min(keys)) > 1, t["name"]
    for t in ORB_GOLD["tie"]:
        o = t["out"]
        keys = [tuple(o[3 * j:3 * j + 3]) for j in range(t["n"])]
        assert len(o) == 3 * t["n"] and keys.count(min(keys)) > 1, t["name"]


def host_lin(c, seeds, tmp):
    f = os.path.join(tmp, c.name + ".sms")
    with open(f, "w") as fh:
        fh.write(synth.sms_text(c.m, c.n, c.ent))
    got = {}
    for s0, n in runs_of(seeds):
        rc, out, err = run([INP, "--gpu", "0", "--costs", "--seed", str(s0), "-O", str(n), f])
        assert rc == 0, (c.name, err)
        lines = [ln.split() for ln in out.splitlines()]
        assert lines[0][0] == "base" and [ln[0] for ln in lines[1:]] == [str(s0 + j) for j in range(n)], c.name
        got[synth.BASE_SEED] = [int(x) for x in lines[0][1:]]
        for j in range(n):
            got[s0 + j] = [int(x) for x in lines[1 + j][1:]]
    return [got[s] for s in seeds]


def test_host_inplacer_equals_golden_every_case(tmp_path):
    assert len(INPLACER_SKIPS) <= 5

    def one(e):
        c = LIN_CASES[e["name"]]
        if c.refusal:                              # the device's refusals run on the host: scored by the oracle here
            rows = lin_oracle.rows_of(c.m, c.n, c.ent)
            return e["name"], host_lin(c, REFUSAL_SEEDS, str(tmp_path)), [lin_oracle.cost6(rows, c.n, s) for s in REFUSAL_SEEDS]
        return e["name"], host_lin(c, e["seeds"], str(tmp_path)), e["out"]

    todo = [e for e in LIN_GOLD["cases"] if e["name"] not in INPLACER_SKIPS]
    with ThreadPoolExecutor(max_workers=8) as ex:
        for name, got, want in ex.map(one, todo):
            assert got == want, name


def host_orbit(c, seeds, tmp, modulus=None, measure=None):
    modulus = c.modulus if modulus is None else modulus
    measure = c.measure if measure is None else measure
    files = []
    for M, x in zip((c.L, c.R, c.P), "LRP"):
        files.append(os.path.join(tmp, "%s_%s.sms" % (c.name, x)))
        with open(files[-1], "w") as fh:
            fh.write(synth.sms_text(*M))
    args = (["-m", str(modulus)] if modulus else []) + (["-c"] if measure == synth.CANONICAL else [])
    got = {}
    for s0, n in runs_of(seeds):
        rc, out, err = run([ORB, "--gpu", "0", "--costs", "--seed", str(s0), "-O", str(n)] + args + files)
        if rc != 0:
            return rc, err
        lines = [[int(x) for x in ln.split()] for ln in out.splitlines()]
        assert len(lines) == n + 1, c.name
        got[synth.BASE_SEED] = lines[0]
        for j in range(n):
            got[s0 + j] = lines[1 + j]
    return 0, [got[s] for s in seeds]


def test_host_orbiter_equals_golden_every_case(tmp_path):
    assert len(ORBITER_SKIPS) <= 5 and all(n in ORB_CASES for n in ORBITER_SKIPS)
    assert all(c.modulus % 2 == 1 for c in ORB_CASES.values() if c.modulus and c.name not in ORBITER_SKIPS)    # -m leaves an odd modulus as it is

    def one(e):
        c = ORB_CASES[e["name"]]
        if c.name == "orbit_refuse_den3_mod9":     # the tool refuses it as the device does
            rc, err = host_orbit(c, REFUSAL_SEEDS, str(tmp_path))
            return e["name"], (rc, "not invertible" in err), (2, True)
        if c.refusal:                              # the device's refusals run on the host: scored by the oracle here
            mats = orbit_mats(c)
            want = [list(orbit_oracle.cost3(mats, c.mkn, s, modulus=c.modulus, measure=c.measure)) for s in REFUSAL_SEEDS]
            return e["name"], host_orbit(c, REFUSAL_SEEDS, str(tmp_path)), (0, want)
        return e["name"], host_orbit(c, e["seeds"], str(tmp_path)), (0, e["out"])

    todo = [e for e in ORB_GOLD["cases"] if e["name"] not in ORBITER_SKIPS]
    with ThreadPoolExecutor(max_workers=8) as ex:
        for name, got, want in ex.map(one, todo):
            assert got == want, name


@pytest.mark.parametrize("name", sorted(LIN_TIE))
def test_host_inplacer_search_on_ties_prints_the_golden_winner(name, tmp_path):
    """the incumbent rule and the order (ADD, SCA, seed, variant) as the tool implements them: its search over the tie
    block's seeds prints the program of the (seed, variant) that lin_oracle.search chose for the golden, byte for byte"""
    T = next(t for t in LIN_GOLD["tie"] if t["name"] == name)
    c = LIN_TIE[name]
    ops, seed, var = T["search"]
    block = [(T["out"][6 * k + 3 * v], T["out"][6 * k + 3 * v + 1], T["seed0"] + k, v) for k in range(T["n"]) for v in (0, 1)]
    if lin_oracle.better(min(block)[:2], T["base"][:2]):   # the stored winner is the block's argmin, or the incumbent when that is no better
        assert (ops[0], ops[1], seed, var) == min(block), name
    else:
        assert (ops, seed, var) == (T["base"][:3], synth.BASE_SEED, 0), name
    f = tmp_path / (name + ".sms")
    f.write_text(synth.sms_text(c.m, c.n, c.ent))
    rc, out, err = run([INP, "--gpu", "0", "--seed", str(T["seed0"]), "-O", str(T["n"]), str(f)])
    assert rc == 0, err
    rows = lin_oracle.rows_of(c.m, c.n, c.ent)
    perm, v = lin_oracle.candidate(rows, c.n, seed)
    assert tuple(v[var][0]) == tuple(ops), name
    assert out == lin_oracle.input2temps(c.n, "i", "z") + lin_oracle.pprint("o", v[var][1], perm), name


@pytest.mark.parametrize("kernel", ["lin", "orbit"])
def test_host_tools_equal_golden_on_the_tie_blocks(kernel, tmp_path):
    if kernel == "lin":
        for t in LIN_GOLD["tie"]:
            seeds = [synth.BASE_SEED] + list(range(t["seed0"], t["seed0"] + t["n"]))
            got = host_lin(LIN_TIE[t["name"]], seeds, str(tmp_path))
            assert got[0] == t["base"] and [x for g in got[1:] for x in g] == t["out"], t["name"]
    else:
        for t in ORB_GOLD["tie"]:
            seeds = [synth.BASE_SEED] + list(range(t["seed0"], t["seed0"] + t["n"]))
            rc, got = host_orbit(ORB_TIE[t["name"]], seeds, str(tmp_path))
            assert rc == 0 and got[0] == t["base"] and [x for g in got[1:] for x in g] == t["out"], t["name"]
