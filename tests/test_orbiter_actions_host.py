"""bin/orbiter --action pluq|householder on the host (--gpu 0): per-seed counts against tests/golden/orbit_action_costs.json
(the literal oracle tests/orbit_action_oracle.py), properties of the candidates that need no oracle (a Householder candidate
keeps every row 2-norm of L and R and every column 2-norm of P; a PLUQ candidate of an integer triple is integral; both keep
the Brent equations), a search per action, and the default action, which prints what no flag prints."""
import json
import os
import shutil
import subprocess
from fractions import Fraction

import pytest

import orbit_action_cases as C
import orbit_oracle as O
import synth
from plo_testlib import DATA, GOLDEN, ROOT, read_sms

ORB = os.path.join(ROOT, "bin", "orbiter")
GOLD = json.load(open(os.path.join(GOLDEN, "orbit_action_costs.json")))
CASES = {c.name: c for c in C.cases()}
ACTIONS = ["pluq", "householder"]


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


def costs(src, action, modulus, measure, seeds):
    """`--costs` of the tool for the seeds, in their order: one run per (seed0, n) run of C.SEED_RUNS"""
    args = ["--gpu", "0", "--action", action, "--costs"] + (["-m", str(modulus)] if modulus else []) + (["-c"] if measure == 2 else [])
    by_seed = {}
    for s0, n in C.SEED_RUNS:
        n = min(n, C.BASE_SEED - s0)                  # the tool's --costs prints the base candidate itself, first
        rc, out, err = run([ORB] + args + ["--seed", str(s0), "-O", str(n)] + src)
        assert rc == 0, err
        lines = [list(map(int, ln.split())) for ln in out.splitlines()]
        assert len(lines) == n + 1
        by_seed[C.BASE_SEED] = lines[0]
        for j in range(n):
            by_seed[s0 + j] = lines[1 + j]
    return [by_seed[s] for s in seeds]


def test_golden_covers_the_issue():
    names = [e["name"] for e in GOLD["cases"]]
    assert names == [c.name for c in C.cases()] + C.FIXTURES
    assert {e["mode"] for e in GOLD["cases"]} == {"list", "runs"}
    for e in GOLD["cases"]:
        want = [C.key(a, p, ms) for a in (C.PLUQ, C.HOUSEHOLDER) for p, ms in C.FIELDS]
        if e["kind"] == "case":
            assert sorted(e["out"]) == sorted(want) and e["sha256"] == CASES[e["name"]].sha256
        else:
            assert set(e["out"]) <= set(want) and all(C.key(a, 0, ms) in e["out"] for a in (C.PLUQ, C.HOUSEHOLDER) for ms in (0, 2))
        assert all(len(v) == len(C.seeds_of(e["mode"])) for v in e["out"].values())
    ds = GOLD["householder_d_by_size"]
    assert all(0 in ds[s] for s in "123") and 3 in ds["3"]


@pytest.mark.parametrize("entry", GOLD["cases"], ids=lambda e: e["name"])
def test_costs_equal_golden(entry, tmp_path):
    """fails without the feature: the tool does not know --action and exits 2"""
    src = files(entry["name"]) if entry["kind"] == "fixture" else write_case(CASES[entry["name"]], tmp_path)
    seeds = C.seeds_of(entry["mode"])
    for key, want in sorted(entry["out"].items()):
        action, mod, ms = key.split("|")
        assert costs(src, action, int(mod), int(ms), seeds) == want, key


def test_oracle_equals_golden_few_seeds():
    """the Fraction oracle recomputes the base candidate and two seeds of one entry per case and action"""
    import orbit_action_oracle as A
    for n, e in enumerate(GOLD["cases"]):
        if e["kind"] == "fixture":
            mats, sh = O.load(os.path.join(DATA, e["name"]))
        else:
            c = CASES[e["name"]]
            mats, sh = [O.dense(*M) for M in (c.L, c.R, c.P)], c.mkn
        seeds = C.seeds_of(e["mode"])
        keys = sorted(e["out"])
        for key in (keys[n % len(keys)], keys[(n + 9) % len(keys)]):
            action, mod, ms = key.split("|")
            for j in (seeds.index(C.BASE_SEED), n % 16, len(seeds) - 2):
                assert list(A.cost3(mats, sh, seeds[j], A.ACTIONS[action], int(mod), int(ms))) == e["out"][key][j], (e["name"], key, seeds[j])


def test_costs_equal_golden_at_the_bound_and_on_ties(tmp_path):
    by_name = {c.name: c for c, _, _ in C.bound_cases()}
    for i, e in enumerate(GOLD["bound"]):
        c = by_name[e["name"]]
        assert c.sha256 == e["sha256"]
        if not e["refused"]:
            assert costs(write_case(c, tmp_path), e["action"], 0, 0, C.seeds_of(e["mode"])) == e["out"], e["name"]
    ties = {(c.name, C.ACTION_NAMES[a]): c for c, a in C.tie_cases()}
    for e in GOLD["tie"]:
        c = ties[(e["name"], e["action"])]
        assert c.sha256 == e["sha256"]
        src = write_case(c, tmp_path)
        args = (["-m", str(c.modulus)] if c.modulus else []) + (["-c"] if c.measure == 2 else [])
        rc, out, err = run([ORB, "--gpu", "0", "--action", e["action"], "--costs", "--seed", str(e["seed0"]), "-O", str(e["n"])] + args + src)
        assert rc == 0, err
        lines = out.splitlines()
        assert list(map(int, lines[0].split())) == e["base"]
        assert [int(x) for ln in lines[1:] for x in ln.split()] == e["out"], (e["name"], e["action"])


def candidate(name, action, seed, d):
    rc, _, err = run([ORB, "--gpu", "0", "--action", action, "--candidate", str(seed), str(d)] + files(name))
    assert rc == 0, err
    return [O.dense(*read_sms(os.path.join(str(d), x + ".sms"))) for x in "LRP"]


def norms(mats):
    """the sorted squared 2-norms of the rows of L, of the rows of R and of the columns of P"""
    L, R, P = mats
    sq = lambda rows: sorted(sum((Fraction(x) ** 2 for x in row), Fraction(0)) for row in rows)  # noqa: E731
    return sq(L), sq(R), sq(O.transpose(P))


@pytest.mark.parametrize("name", ["2x2x2_7_Winograd", "4x4x4_48_rational"])
def test_householder_keeps_every_row_and_column_norm(name, tmp_path):
    want = norms([O.dense(*read_sms(f)) for f in files(name)])
    moved = 0
    for seed in range(16):
        got = candidate(name, "householder", seed, tmp_path / str(seed))
        assert norms(got) == want, seed
        moved += [[list(r) for r in M] for M in got] != [[list(r) for r in O.dense(*read_sms(f))] for f in files(name)]
    assert moved >= 8                                   # the candidates are not the input again


@pytest.mark.parametrize("name", ["2x2x2_7_Winograd", "4x4x4_49_156"])
def test_pluq_of_an_integer_triple_is_integral(name, tmp_path):
    assert all(Fraction(x).denominator == 1 for f in files(name) for x in read_sms(f)[2].values())
    for seed in range(16):
        got = candidate(name, "pluq", seed, tmp_path / str(seed))
        assert all(Fraction(x).denominator == 1 for M in got for row in M for x in row), seed


@pytest.mark.parametrize("action", ACTIONS)
def test_candidates_keep_the_brent_equations(action, tmp_path):
    for name, seeds in (("2x2x2_7_Winograd", range(16)), ("3x3x3_23_58", (0, 7))):
        mats, sh = O.load(os.path.join(DATA, name))
        assert O.mm_check(*mats, sh)
        for seed in seeds:
            assert O.mm_check(*candidate(name, action, seed, tmp_path / ("%s_%d" % (name, seed))), sh), (name, seed)


@pytest.mark.parametrize("action", ACTIONS)
@pytest.mark.parametrize("name,args", [("2x2x2_7_Winograd", []), ("3x3x3_23_58", ["-m", "131071"])])
def test_search_of_two_thousand_candidates(action, name, args, tmp_path):
    for f in files(name):
        shutil.copy(f, tmp_path)
    src = files(name, str(tmp_path))
    rc, out, err = run([ORB, "--gpu", "0", "--action", action, "-O", "2000"] + args + src)
    assert rc == 0, err
    assert "restarts on host" in err and out.startswith("winner ")
    outs = [p[:-4] + ".nnz.sms" for p in src]
    mod = int(args[1]) if args else 0
    if out.split()[4] == "base":
        assert not any(os.path.exists(p) for p in outs)
    else:
        got = [O.dense(*read_sms(p)) for p in outs]
        mats, sh = O.load(os.path.join(DATA, name))
        assert O.mm_check(*got, sh, modulus=mod)
        assert O.counts(*got, modulus=mod) == tuple(int(x) for x in out.split()[1:4])
        assert O.counts(*got, modulus=mod) < O.counts(*mats, modulus=mod)


def test_action_triangular_prints_what_no_flag_prints(tmp_path):
    name = "4x4x4_49_156"
    a = run([ORB, "--gpu", "0", "--costs", "-O", "50"] + files(name))
    b = run([ORB, "--gpu", "0", "--action", "triangular", "--costs", "-O", "50"] + files(name))
    assert a[0] == 0 and a[:2] == b[:2]
    outs = []
    for i, extra in enumerate(([], ["--action", "triangular"])):
        d = tmp_path / str(i)
        d.mkdir()
        for f in files("2x2x2_7_Winograd"):
            shutil.copy(f, d)
        src = files("2x2x2_7_Winograd", str(d))
        rc, out, err = run([ORB, "--gpu", "0", "-O", "300"] + extra + src)
        assert rc == 0, err
        outs.append((out, [open(p[:-4] + ".nnz.sms", "rb").read() for p in src]))
    assert outs[0] == outs[1]


def test_unknown_action_exits_2_and_usage_names_the_flag():
    rc, out, err = run([ORB, "--gpu", "0", "--action", "givens", "-O", "5"] + files("2x2x2_7_Winograd"))
    assert rc == 2 and "ERROR" in err and not out
    rc, out, err = run([ORB, "-h"])
    assert "--action triangular|pluq|householder" in err
