"""The synthetic edge cases of tests/synth.py (lin_cases, orbit_cases, kmethod_cases, tril_cases) without a device: the
generators still produce the inputs the goldens were made from (SHA-256), the oracles recompute the goldens' quick cases, and
the HOST engines (plo_inplace.hpp through `bin/inplacer --gpu 0 --costs`, plo_orbit.hpp through `bin/orbiter --gpu 0 --costs`)
give the goldens' counts on every case -- the cases the device refuses included, which the oracle scores here.
`bin/trilplacer` has no `--costs`: its host engine is held to the trilinear goldens through the winner it prints for seeds
0..7; `bin/optimizer -K` prints no per-restart counts of the decomposition the goldens record, so the kernel method's host
path is not held to them here."""
import importlib.util
import json
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import lin_oracle
import orbit_oracle
import synth
from plo_testlib import GOLDEN, ROOT, OracleMatrix, OracleTril

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


# ---------------------------------------------------------------------------------------------------- kernel method, trilinear
TRP = os.path.join(ROOT, "bin", "trilplacer")
KM_GOLD = json.load(open(os.path.join(GOLDEN, "kmethod_synth_costs.json")))
TRIL_GOLD = json.load(open(os.path.join(GOLDEN, "tril_synth_costs.json")))
KM_CASES = {c.name: c for c in synth.kmethod_cases()}
TRIL_CASES = {c.name: c for c in synth.tril_cases()}
TRIL_TIE = {c.name: c for c in synth.tril_tie_cases()}


def oracle_tril(c):
    (na, A), (nb, B), (nt, T) = c.mats
    return OracleTril((c.m, na, A), (c.m, nb, B), (nt, c.m, {(j, i): v for (i, j), v in T.items()}))


def test_kmethod_tril_generators_reproduce_the_goldens_inputs():
    for gold, cases in ((KM_GOLD, KM_CASES), (TRIL_GOLD, TRIL_CASES)):
        assert [e["name"] for e in gold["cases"]] == list(cases)
        for e in gold["cases"]:
            c = cases[e["name"]]
            assert c.sha256 == e["sha256"] and c.family == e["family"], e["name"]
            assert e.get("refusal") == c.refusal, e["name"]
            if not c.refusal:
                assert (e["mode"], e["seeds"], e["quick"]) == (c.mode, c.seeds, c.quick), e["name"]
                assert len(e["out"]) == len(e["seeds"]) and set(e["seeds"]) <= set(synth.SEEDS_LIST)
    assert all(e["mode"] == "runs" and e["seeds"] == synth.SEEDS_RUNS and e["p"] == KM_CASES[e["name"]].p for e in KM_GOLD["cases"] if "mode" in e)
    modes = [e["mode"] for e in TRIL_GOLD["cases"] if "mode" in e]
    assert abs(modes.count("list") - modes.count("runs")) <= 2
    assert [len(e["seeds"]) for e in TRIL_GOLD["cases"] if "mode" in e].count(3) == 2          # the two programs near 160 KiB
    assert [t["name"] for t in TRIL_GOLD["tie"]] == list(TRIL_TIE)
    for t in TRIL_GOLD["tie"]:
        assert TRIL_TIE[t["name"]].sha256 == t["sha256"] and (t["seed0"], t["n"]) == (synth.TIE_SEED0, synth.TRIL_TIE_N), t["name"]
    B = KM_GOLD["per_block"]
    assert (B["seed0"], B["n"], B["per_block"]) == synth.KM_PER_BLOCK and B["name"] in KM_CASES and not KM_CASES[B["name"]].unit
    assert len(KM_CASES) >= 45 and len(TRIL_CASES) >= 65


def test_generated_kmethod_tril_cases_are_what_the_issue_names():
    """the edges by name: a failure of a family names its edge"""
    fam = lambda cases, f: [c for c in cases.values() if c.family == f]  # noqa: E731
    a = fam(KM_CASES, "a")
    assert sorted((c.m, c.n) for c in a) == [(4, 2), (64, 32), (64, 32), (68, 34), (127, 64), (128, 64)]
    top = KM_CASES["km_a_128x64"]
    assert (top.m, top.n, top.rank, top.m - top.rank) == (128, 64, 64, 64)                       # the three limits at once
    assert all(c.unit for c in KM_CASES.values() if c.m > 64 and not c.refusal)
    assert sorted((c.m, c.n, c.m - c.rank) for c in fam(KM_CASES, "b")) == [(40, 3, 39), (65, 1, 64), (66, 2, 64), (68, 4, 64)]
    c_ = [c for c in fam(KM_CASES, "c") if c.name != "km_c_64x16_dense"]
    assert sorted({c.rank for c in c_}) == synth.KM_R and all(c.m == c.rank + 1 and len(c.rows[-1]) == c.rank for c in c_)
    assert {max(2, (c.rank - 1).bit_length()) for c in c_} == {2, 3, 4, 5, 6}                   # Dep's lpr_log2 (layout_plan: from the rank)
    assert len(c_) == 2 * len(synth.KM_R) - 1 and max(len(r) for r in KM_CASES["km_c_R64_ones"].rows) == 64
    d = fam(KM_CASES, "d")
    assert sum(1 for c in d if any(not r for r in c.rows)) == 2 and KM_CASES["km_d_3x2_empty"].rows[-1] == {}
    assert all(j % 2 == 0 for r in KM_CASES["km_d_12x16_even"].rows for j in r) and KM_CASES["km_d_12x16_even"].rank == 8
    c63 = KM_CASES["km_d_64x64_col63"]
    assert c63.p == 2147483629 and all(len(r) == 3 and max(r) < 63 for r in c63.rows)
    assert [c.p for c in fam(KM_CASES, "e")] == synth.KM_MODULI and all((c.m, c.n) == (30, 12) for c in fam(KM_CASES, "e"))
    assert {c.name: c.refusal for c in fam(KM_CASES, "refuse")} == {
        "km_refuse_67x2_65dep": "PLO_E_UNSUPPORTED", "km_refuse_128x64_rank62": "PLO_E_UNSUPPORTED", "km_refuse_129x2": "PLO_E_UNSUPPORTED",
        "km_refuse_3x65": "PLO_E_UNSUPPORTED", "km_refuse_4x7_fullrank": "PLO_E_UNSUPPORTED", "km_refuse_3x2_allempty": "PLO_E_UNSUPPORTED",
        "km_refuse_65x3_a2": "PLO_E_CAPACITY"}
    r62 = KM_CASES["km_refuse_128x64_rank62"]
    assert (r62.m, r62.n, r62.rank) == (128, 64, 62) and all(len(r) == 2 for r in r62.rows) and r62.unit

    lens = lambda c, w: sorted(sum(1 for (r, _) in c.mats[w][1] if r == i) for i in range(c.m))  # noqa: E731
    assert sorted({c.m for c in fam(TRIL_CASES, "a")}) == [1, 2, 63, 64, 65, 129]
    assert all(len({n for n, _ in c.mats}) == 3 and all(3 <= n <= 9 for n, _ in c.mats) for c in fam(TRIL_CASES, "a"))
    for w, x in enumerate("ABT"):                                                                # a row of 64 entries in each of A, B, T alone
        only = [c for c in fam(TRIL_CASES, "b") if c.name.startswith("tril_b_row64_%s_" % x)]
        assert len(only) == 4 and all([lens(c, v)[-1] == 64 for v in range(3)] == [v == w for v in range(3)] for c in only)
    assert all(lens(c, w)[-1] == 64 for c in fam(TRIL_CASES, "b") if "row64_ABT" in c.name for w in range(3))
    assert all(lens(c, w)[-1] == 1 for c in fam(TRIL_CASES, "b") if "len1" in c.name for w in range(3))
    assert all(c.m == 1 and c.expanded and lens(c, 2) == [64] for c in fam(TRIL_CASES, "b") if "m1_T64" in c.name)
    assert all(c.expanded for c in fam(TRIL_CASES, "c")) and [c.unit for c in fam(TRIL_CASES, "c")] == [True, False]
    for c in fam(TRIL_CASES, "d"):                                                               # variable 16381 in A, B and (the expansion of) T
        assert [n for n, _ in c.mats] == [16382, 16382, 16381 if c.expanded else 16382]
        assert all({0, n - 1} <= {j for (_, j) in e} for n, e in c.mats)
    e_ = {c.name: c for c in fam(TRIL_CASES, "e")}
    assert sorted(c.waves for c in e_.values()) == [1] * 8 + [4] * 4
    assert all(4 * c.lds_per_wave <= synth.WG_LDS for n, c in e_.items() if "under64k" in n) and all(4 * c.lds_per_wave > synth.WG_LDS for n, c in e_.items() if "over64k" in n)
    assert (e_["tril_e_1200x200_unit"].m, e_["tril_e_600x200_rat_e"].m, e_["tril_e_300x64_unit"].m, e_["tril_e_200x64_rat_e"].m) == (1200, 600, 300, 200)
    for f, per in (("a", 6), ("d", 1)):                                                         # the four variants: +-1 and rational, plain and -e
        assert sorted((c.unit, c.expanded) for c in fam(TRIL_CASES, f)) == sorted([(u, x) for u in (False, True) for x in (False, True)] * per)
    assert {c.name: c.refusal for c in fam(TRIL_CASES, "refuse")} == {
        "tril_refuse_empty_row": "PLO_E_UNSUPPORTED", "tril_refuse_row65": "PLO_E_UNSUPPORTED", "tril_refuse_T16382_e": "PLO_E_CAPACITY",
        "tril_refuse_num_prime": "PLO_E_UNSUPPORTED", "tril_refuse_den_prime": "PLO_E_UNSUPPORTED", "tril_refuse_m16383": "PLO_E_CAPACITY"}


def test_c_oracle_recomputes_the_kmethod_cases():
    quick = [e for e in KM_GOLD["cases"] if e.get("quick")]
    assert len(quick) == sum(1 for c in KM_CASES.values() if not c.refusal) >= 40
    for e in quick:
        c = KM_CASES[e["name"]]
        M = OracleMatrix(*c.csr, c.p)
        assert [list(M.kernel_restart(s)) for s in e["seeds"]] == e["out"], e["name"]
        assert all(o[2] == c.rank and o[3] + o[4] == c.m - c.rank for o in e["out"]), e["name"]   # rank, NotIndep + kept = dependent rows
    B = KM_GOLD["per_block"]
    c = KM_CASES[B["name"]]
    M = OracleMatrix(*c.csr, c.p)
    assert [list(M.kernel_restart(s)) for s in B["seeds"]] == B["out"]


def test_c_oracle_recomputes_the_quick_tril_cases():
    quick = [e for e in TRIL_GOLD["cases"] if e.get("quick")]
    assert len(quick) >= 55 and max(TRIL_CASES[e["name"]].m for e in quick) == 300 and any(TRIL_CASES[e["name"]].family == "d" for e in quick)
    for e in quick:
        c = TRIL_CASES[e["name"]]
        assert [list(a) + list(b) for a, b in oracle_tril(c).cost_many(seeds=e["seeds"], expanded=c.expanded)] == e["out"], e["name"]
        assert all(o[2] == o[5] == c.m for o in e["out"]), e["name"]                             # one AXPY per row


def test_tril_tie_blocks_tie():
    for t in TRIL_GOLD["tie"]:
        o = t["out"]
        keys = [(o[6 * k + 3 * v], o[6 * k + 3 * v + 1], t["seed0"] + k, v) for k in range(t["n"]) for v in (0, 1)]
        assert len(o) == 6 * t["n"] and [k[:2] for k in keys].count(min(keys)[:2]) > 1, t["name"]
        best = min(keys)
        assert t["search"] == [[best[0], best[1], o[6 * (best[2] - t["seed0"]) + 3 * best[3] + 2]], best[2], best[3]], t["name"]


def host_tril_winner(c, seed0, n, tmp):
    """(base counts, (counts, seed, variant) of the winner or None when the unpermuted program stays) as bin/trilplacer --gpu 0 prints them"""
    (na, A), (nb, B), (nt, T) = c.mats
    files = []
    for x, M in (("L", (c.m, na, A)), ("R", (c.m, nb, B)), ("P", (nt, c.m, {(j, i): v for (i, j), v in T.items()}))):
        files.append(os.path.join(tmp, "%s_%s.sms" % (c.name, x)))
        with open(files[-1], "w") as fh:
            fh.write(synth.sms_text(*M))
    rc, out, err = run([TRP, "--gpu", "0", "--seed", str(seed0), "-O", str(n)] + (["-e"] if c.expanded else []) + files)
    assert rc == 0 and "restarts on host" in err, (c.name, err)
    base = re.search(r"# Oriented number of operations: (\d+)\|(\d+)\|(\d+)", err)
    found = re.search(r"# Found (oriented|unoriented) \[seed (\d+)\], operations: (\d+)\|(\d+)\|(\d+)", err)
    final = [int(x) for x in re.findall(r"(\d+)\t(?:ADD|SCA|AXPY)", err)]
    win = ([int(found.group(k)) for k in (3, 4, 5)], int(found.group(2)), int(found.group(1) == "unoriented")) if found else None
    assert final == (win[0] if win else [int(x) for x in base.groups()]), c.name
    return [int(x) for x in base.groups()], win


def tril_want(base, ops, seeds):
    """the rule of the tool: the loop's best under (ADD, SCA, seed, variant), kept only when strictly better than the unpermuted program"""
    best = min((o[3 * v], o[3 * v + 1], s, v) for s, o in zip(seeds, ops) for v in (0, 1))
    o = ops[seeds.index(best[2])]
    return (o[3 * best[3]:3 * best[3] + 3], best[2], best[3]) if best[:2] < tuple(base[:2]) else None


def test_host_trilplacer_winner_equals_golden_every_quick_case(tmp_path):
    """seeds 0..7 are among every case's seeds, and BASE_SEED is the unpermuted oriented program the tool starts from"""
    def one(e):
        c = TRIL_CASES[e["name"]]
        by_seed = dict(zip(e["seeds"], e["out"]))
        base = by_seed[synth.BASE_SEED][:3]
        return e["name"], host_tril_winner(c, 0, 8, str(tmp_path)), (base, tril_want(base, [by_seed[s] for s in range(8)], list(range(8))))

    todo = [e for e in TRIL_GOLD["cases"] if e.get("quick")]
    with ThreadPoolExecutor(max_workers=8) as ex:
        for name, got, want in ex.map(one, todo):
            assert got == want, name


@pytest.mark.parametrize("name", sorted(TRIL_TIE))
def test_host_trilplacer_search_on_ties_prints_the_golden_winner(name, tmp_path):
    T = next(t for t in TRIL_GOLD["tie"] if t["name"] == name)
    base, win = host_tril_winner(TRIL_TIE[name], T["seed0"], T["n"], str(tmp_path))
    assert win is not None and [win[0], win[1], win[2]] == T["search"], name


# ---------------------------------------------------------------------------------------------------- the one-wave CSE kernel
def test_cse_generators_reproduce_the_pinned_cases():
    """names, shapes and matrices of synth.cse_cases() (tests/golden/make_cse_cases.py); the oracle scores them live"""
    spec = importlib.util.spec_from_file_location("make_cse_cases", os.path.join(GOLDEN, "make_cse_cases.py"))
    make_cse_cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make_cse_cases)
    gold = json.load(open(os.path.join(GOLDEN, "cse_cases.json")))["cases"]
    cases = synth.cse_cases()
    assert [e["name"] for e in gold] == [c.name for c in cases] and len(cases) == 89
    for e, c in zip(gold, cases):
        assert e == make_cse_cases.entry(c), e["name"]
    assert [e["name"] for e in gold if "refusal" in e] == ["cse_rowlen_L65_unit", "cse_moduli_key53_8x1023"]
