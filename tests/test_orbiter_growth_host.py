"""bin/orbiter -g on the host (--gpu 0): the growth factor of every candidate, bit for bit, against
tests/golden/orbit_growth_costs.json (the literal oracle tests/orbit_growth_oracle.py, which this file recomputes where it is
quick), the refusals, the winner's files, and the improvement the search finds from 2x2x2_7_Winograd."""
import json
import os
import re
import shutil
import subprocess

import pytest

import orbit_growth_cases as C
import orbit_growth_oracle as G
import orbit_oracle as O
import synth
from plo_testlib import DATA, GOLDEN, ROOT

ORB = os.path.join(ROOT, "bin", "orbiter")
GF = os.path.join(ROOT, "bin", "growthfactor")
GOLD = json.load(open(os.path.join(GOLDEN, "orbit_growth_costs.json")))
ACTIONS = ["triangular", "pluq"]
ACT = {"triangular": 0, "pluq": 1}
HOST_IDX = [C.SEEDS.index(s) for s in C.HOST_SEEDS]       # where the host seeds stand among the golden's


def run(cmd, timeout=300):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout, r.stderr


def files(name, d=DATA):
    return [os.path.join(d, "%s_%s.sms" % (name, x)) for x in "LRP"]


def write_case(c, d):
    os.makedirs(str(d), exist_ok=True)
    out = files(c.name, str(d))
    for path, M in zip(out, (c.L, c.R, c.P)):
        with open(path, "w") as f:
            f.write(synth.sms_text(*M))
    return out


def parse(line):
    cost, nnz, nno = line.split()
    return ["%016x" % G.bits(float(cost)), int(nnz), int(nno)]


def costs(src, action):
    """`-g --costs` for C.HOST_SEEDS: the base candidate and seeds 0 .. 31 in one run, 2^40 in another"""
    res = []
    for s0, n in ((0, 32), (1 << 40, 1)):
        rc, out, err = run([ORB, "-g", "--gpu", "0", "--action", action, "--costs", "--seed", str(s0), "-O", str(n)] + src)
        assert rc == 0, err
        lines = [parse(ln) for ln in out.splitlines()]
        assert len(lines) == n + 1
        res += lines if s0 == 0 else lines[1:]
    return res


def synth_cases():
    seen, out = set(), []
    for c in synth.orbit_cases():
        text = "".join(synth.sms_text(*M) for M in (c.L, c.R, c.P))
        if c.modulus == 0 and text not in seen:
            seen.add(text)
            out.append(c)
    return out


SYNTH = {c.name: c for c in synth_cases()}
CASES = {c.name: c for c in C.cases()}
BOUND = {c.name: (c, a, r) for c, a, r in C.bound_cases()}


def test_golden_covers_the_issue():
    assert GOLD["seeds"] == C.SEEDS and GOLD["host_seeds"] == C.HOST_SEEDS
    assert [e["name"] for e in GOLD["fixtures"]] == C.FIXTURES
    assert [(e["name"], e["sha256"]) for e in GOLD["cases"]] == [(c.name, c.sha256) for c in C.cases()]
    assert [(e["name"], e["sha256"], e["action"], e["refused"]) for e in GOLD["bound"]] == [(c.name, c.sha256, C.ACTION_NAMES[a], r) for c, a, r in C.bound_cases()]
    assert [(e["name"], e["sha256"]) for e in GOLD["synth"]] == [(c.name, c.sha256) for c in synth_cases()] and len(GOLD["synth"]) >= 20
    for e in GOLD["fixtures"] + GOLD["cases"]:
        assert sorted(e["out"]) == sorted(ACTIONS) and all(len(v) == len(C.SEEDS) for v in e["out"].values())
    for e in GOLD["synth"]:
        assert sorted(e["out"]) == sorted(ACTIONS) and all(len(v) == len(C.HOST_SEEDS) for v in e["out"].values())
    assert all(len(e["out"]) == len(C.SEEDS) for e in GOLD["bound"])
    for e in GOLD["cases"]:
        assert e["refusal"] == {an: C.growth_refusal(CASES[e["name"]], a) for a, an in C.ACTION_NAMES.items()}
    # what the cases are there for: r = 63, 64, 65, a term that is zero, an input PLUQ cannot take, rows with several denominators
    assert {CASES[n].r for n in CASES} >= {1, 63, 64, 65}
    assert any(v == "PLO_E_UNSUPPORTED" for e in GOLD["cases"] for v in e["refusal"].values())
    assert any(len({v.denominator for _, v in row}) > 1 for row in synth.orbit_rows(CASES["orbit_growth_2x3x4_rats"]))


@pytest.mark.parametrize("entry", GOLD["fixtures"], ids=lambda e: e["name"])
def test_fixture_costs_equal_golden(entry):
    """fails without the feature: the tool does not know -g and exits 2"""
    for action in ACTIONS:
        assert costs(files(entry["name"]), action) == [entry["out"][action][i] for i in HOST_IDX], action


@pytest.mark.parametrize("entry", GOLD["synth"], ids=lambda e: e["name"])
def test_synth_costs_equal_golden(entry, tmp_path):
    """the triples over Q of synth.orbit_cases(): those beyond the device's limits or its 2^53 proof are scored like the others"""
    src = write_case(SYNTH[entry["name"]], tmp_path)
    for action in ACTIONS:
        assert costs(src, action) == entry["out"][action], action


@pytest.mark.parametrize("entry", GOLD["cases"] + GOLD["bound"], ids=lambda e: e["name"])
def test_edge_costs_equal_golden(entry, tmp_path):
    c = CASES[entry["name"]] if entry["name"] in CASES else BOUND[entry["name"]][0]
    src = write_case(c, tmp_path)
    for action in ([entry["action"]] if "action" in entry else ACTIONS):
        want = entry["out"] if "action" in entry else entry["out"][action]
        assert costs(src, action) == [want[i] for i in HOST_IDX], action


def test_oracle_equals_golden_where_it_is_quick():
    """the literal oracle again: three seeds of every fixture, edge case and quick synthetic triple, both actions"""
    def check(mats, mkn, action, want, seeds):
        for j in (0, 1 + len(want) % 7, len(want) - 1):
            c = G.cost3(mats, mkn, seeds[j], ACT[action])
            assert ["%016x" % G.bits(c[0]), c[1], c[2]] == want[j]
    for e in GOLD["fixtures"]:
        mats, mkn = O.load(os.path.join(DATA, e["name"]))
        for a in ACTIONS:
            check(mats, mkn, a, e["out"][a], C.SEEDS)
    for e in GOLD["cases"] + GOLD["bound"] + [e for e in GOLD["synth"] if e["quick"]]:
        c = CASES.get(e["name"]) or SYNTH.get(e["name"]) or BOUND[e["name"]][0]
        mats = [O.dense(*M) for M in (c.L, c.R, c.P)]
        for a in ([e["action"]] if "action" in e else ACTIONS):
            want = e["out"] if "action" in e else e["out"][a]
            check(mats, c.mkn, a, want, C.SEEDS if len(want) == len(C.SEEDS) else C.HOST_SEEDS)


def test_base_candidate_is_the_g2_of_growthfactor():
    """the two tools agree on the input: -g's base cost, printed with six decimals, is the G2 line of bin/growthfactor"""
    for name in C.FIXTURES:
        rc, out, err = run([ORB, "-g", "--gpu", "0", "--costs", "-O", "0"] + files(name))
        assert rc == 0, err
        rc, _, gf = run([GF] + files(name))
        assert rc == 0
        assert "%.6f" % float(out.split()[0]) == re.search(r"^## G2:\t\t(\S+)\t", gf, re.M).group(1)


def test_refusals():
    src = files("2x2x2_7_Winograd")
    for extra in (["-q", "131071"], ["-m", "7"], ["-r", "2", "17", "1"], ["-z"], ["-z", "-q", "131071"], ["--action", "householder"]):
        rc, out, err = run([ORB, "-g", "--gpu", "0", "-O", "10"] + extra + src)
        assert rc == 2 and "ERROR" in err and out == "", extra


@pytest.mark.parametrize("action", ACTIONS)
def test_winner_files_pass_the_check(action, tmp_path):
    for f in files("2x2x2_7_Winograd"):
        shutil.copy(f, tmp_path)
    src = files("2x2x2_7_Winograd", str(tmp_path))
    rc, out, err = run([ORB, "-g", "--gpu", "0", "--action", action, "-O", "200"] + src)
    assert rc == 0, err
    assert err.count("SUCCESS: correct 2x2x2") == 2 and "# Init. ops: 17.853007, (42,0)" in err
    _, cost, nnz, nno, seed = out.split()
    assert re.search(r"Rdcd\. opt: %.6f<17\.853007\t\(%s,%s\)" % (float(cost), nnz, nno), err)
    new = [p[:-4] + ".nnz.sms" for p in src]
    # the written triple is a matrix-multiplication algorithm, its own base cost is the winner's, and bin/growthfactor says the same
    rc, out2, err2 = run([ORB, "-g", "--gpu", "0", "-O", "0"] + new)
    assert rc == 0 and "SUCCESS: correct 2x2x2" in err2
    assert out2.split()[:4] == ["winner", cost, nnz, nno]
    rc, _, gf = run([GF] + new)
    assert rc == 0 and "## G2:\t\t%.6f\t" % float(cost) in gf


def test_search_improves_on_winograd(tmp_path):
    """From 2x2x2_7_Winograd (G2 17.8530; Strassen's 14.8284 is in the same orbit) the host loop from seed 0 returns a smaller cost
    already at -O 1, the smallest power of ten: seed 0 itself.  Pinned: the count and the winner's (bits, nnz, nno, seed)."""
    for f in files("2x2x2_7_Winograd"):
        shutil.copy(f, tmp_path)
    src = files("2x2x2_7_Winograd", str(tmp_path))
    rc, out, err = run([ORB, "-g", "--gpu", "0", "--costs", "-O", "0"] + src)
    assert rc == 0
    base = float(out.split()[0])
    rc, out, err = run([ORB, "-g", "--gpu", "0", "-O", "1"] + src)
    assert rc == 0, err
    _, cost, nnz, nno, seed = out.split()
    assert float(cost) < base
    assert ("%016x" % G.bits(float(cost)), int(nnz), int(nno), int(seed)) == ("4030ba5919a791a3", 40, 0, 0)
