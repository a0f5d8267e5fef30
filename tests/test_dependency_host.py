"""bin/dependency on the host (--gpu 0), held to the literal oracle tests/dependency_oracle.py through
tests/golden/dependency_hits.json (made by tests/golden/make_dependency_hits.py): the stdout text of every fixture case, the
coefficient line, the levels, zero and duplicated rows, the refusal of a bad denominator, and a pipeline from bin/optimizer."""
import hashlib
import json
import os
import subprocess

import pytest

import dependency_oracle as D
from plo_testlib import DATA, GOLDEN, ROOT

DEP = os.path.join(ROOT, "bin", "dependency")
GOLD = json.load(open(os.path.join(GOLDEN, "dependency_hits.json")))
# the prototype's counts: (input, -l, -c, -q) -> (combinations, zero, canonical)
TABLE = {
    ("2x2x2_7_Winograd_L", 4, 11, 0): (51051, 6, 233), ("2x2x2_7_Winograd_P", 4, 11, 0): (1881, 0, 0),
    ("2x2x2_7_DPS-accurate_L", 3, 11, 0): (4466, 3, 25), ("3x3x3_23_58_L", 3, 3, 0): (16698, 13, 100),
    ("4x4x4_48_rational_L", 2, 11, 0): (12408, 0, 16), ("3x4x7_63_rational_R", 2, 7, 0): (13671, 0, 45),
    ("4x4x4_49_156_L", 3, 5, 0): (466480, 42, 208), ("2x2x2_7_Winograd_L", 4, 11, 7): (8946, 6, 151),
    ("2x2x2_7_Strassen_L", 4, 11, 3): (462, 6, 46),
}


def run(cmd, stdin=None, timeout=300):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, input=stdin)
    return r.returncode, r.stdout, r.stderr


def args_of(rec, gpu="0"):
    return [DEP, "--gpu", gpu, "-l", str(rec["l"]), "-c", str(rec["c"])] + (["-q", str(rec["q"])] if rec["q"] else []) + (["-v", rec["v"]] if rec["v"] else [])


def input_of(rec, tmp_path):
    if "sms" not in rec:
        return os.path.join(DATA, rec["input"] + ".sms")
    p = tmp_path / (rec["input"] + ".sms")
    p.write_text(rec["sms"])
    return str(p)


def same_text(out, rec):
    if "text" in rec:
        assert out == rec["text"]
    assert out.count("\n") == rec["lines"]
    assert hashlib.sha256(out.encode()).hexdigest() == rec["sha256"]


def case_id(rec):
    return "%s-l%d-c%d-q%d%s" % (rec["input"], rec["l"], rec["c"], rec["q"], "-v" if rec["v"] else "")


def test_golden_holds_the_table():
    seen = {(r["input"], r["l"], r["c"], r["q"]): r for r in GOLD["fixtures"] if not r["v"]}
    for key, (_, zero, cano) in TABLE.items():
        assert (seen[key]["zero"], seen[key]["canonical"]) == (zero, cano), key
        assert seen[key]["lines"] == zero + cano


@pytest.mark.parametrize("rec", GOLD["fixtures"], ids=case_id)
def test_text_equals_golden(rec, tmp_path):
    rc, out, err = run(args_of(rec) + [input_of(rec, tmp_path)])
    assert rc == 0, err
    same_text(out, rec)
    assert rec["head"] in err.splitlines()
    assert "combinations on host" in err
    key = (rec["input"], rec["l"], rec["c"], rec["q"])
    if key in TABLE and not rec["v"]:
        assert "# %d combinations on host" % TABLE[key][0] in err


def test_oracle_equals_golden_small_cases():
    """the Fraction oracle reruns the cases that take it well under a second"""
    for rec in GOLD["fixtures"]:
        if rec["input"].startswith("2x2x2") and rec["l"] <= 3:
            m, n, rows = D.load_sms(os.path.join(DATA, rec["input"] + ".sms"))
            head, hits = D.depender(m, n, rows, level=rec["l"], maxnum=rec["c"], extra=rec["v"].split(), q=rec["q"])
            assert head == rec["head"] and D.text_of(hits) == rec["text"]


@pytest.mark.parametrize("extra,want", [
    (["-l", "2"], "[1,-1,2,-2,1/2,-1/2,3,-3,1/3,-1/3,4]"),
    # 3 and 1/2 are listed already: 2 still brings 2, -2, 1/2, -1/2 (the second 1/2 goes when the list is mapped), 3 brings nothing,
    # 4 brings 4, -4, 1/4, -1/4, and the cut at 11 raw entries drops -1/4
    (["-l", "2", "-v", "3 1/2"], "[1,-1,3,1/2,2,-2,-1/2,4,-4,1/4]"),
    (["-l", "2", "-c", "1"], "[1]"),
    (["-l", "2", "-c", "4", "-q", "7"], "[1,6,2,5]"),
    (["-l", "2", "-c", "6", "-q", "3"], "[1,2]"),
])
def test_coefficient_line(extra, want):
    f = os.path.join(DATA, "2x2x2_7_Strassen_L.sms")
    rc, out, err = run([DEP, "--gpu", "0"] + extra + [f])
    assert rc == 0, err
    m, n, rows = D.load_sms(f)
    o = dict(zip(extra[::2], extra[1::2]))
    head, hits = D.depender(m, n, rows, level=2, maxnum=int(o.get("-c", 11)), extra=o.get("-v", "").split(), q=int(o.get("-q", 0)))
    assert head == "# [DEPND] level 2, coefficients: " + want
    assert head in err.splitlines()
    assert out == D.text_of(hits)


def test_level_one_prints_nothing():
    rc, out, err = run([DEP, "--gpu", "0", "-l", "1", os.path.join(DATA, "2x2x2_7_Winograd_L.sms")])
    assert rc == 0 and out == "" and "# [DEPND] o6" in err and "# 0 combinations" in err


@pytest.mark.parametrize("rec", [r for r in GOLD["synthetic"] if r["input"] in ("zero_and_duplicate_rows", "m1", "m2_level_above_m", "sizes234")], ids=case_id)
def test_synthetic_rows(rec, tmp_path):
    rc, out, err = run(args_of(rec) + [input_of(rec, tmp_path)])
    assert rc == 0, err
    same_text(out, rec)
    if rec["input"] == "zero_and_duplicate_rows" and rec["q"] == 0:
        assert "+o0-o3;\n" in out and "+o0+o1-o3;\n" in out         # the duplicate, and the zero row riding along


def test_reads_stdin():
    rec = GOLD["fixtures"][0]
    text = open(os.path.join(DATA, rec["input"] + ".sms")).read()
    rc, out, err = run(args_of(rec), stdin=text)
    assert rc == 0, err
    same_text(out, rec)


def test_bad_denominator_modulo_q_exits_2(tmp_path):
    p = tmp_path / "third.sms"
    p.write_text("2 2 R\n1 1 1/3\n1 2 1\n2 1 1\n2 2 2\n0 0 0\n")
    rc, out, err = run([DEP, "--gpu", "0", "-q", "3", str(p)])
    assert rc == 2 and out == "" and "ERROR" in err
    rc, out, err = run([DEP, "--gpu", "0", "-q", "7", str(p)])
    assert rc == 0, err


def test_pipeline_from_optimizer():
    """bin/optimizer | bin/SLPchecker | bin/dependency, the shape of the reference's chartreuse workflow"""
    f = os.path.join(DATA, "2x2x2_7_Winograd_L.sms")
    rc, prog, err = run([os.path.join(ROOT, "bin", "optimizer"), "-O", "10", f])
    assert rc == 0 and ":=" in prog, err
    rc, sms, err = run([os.path.join(ROOT, "bin", "SLPchecker")], stdin=prog)
    assert rc == 0, err
    rc, out, err = run([DEP, "--gpu", "0", "-l", "2"], stdin=sms)
    assert rc == 0, err
    m, n, rows = D.parse_sms(sms)
    head, hits = D.depender(m, n, rows, level=2)
    assert head in err.splitlines() and out == D.text_of(hits)
    assert m == 7 and n == 4
