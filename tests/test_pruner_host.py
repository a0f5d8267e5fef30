"""bin/pruner on the host (--gpu 0): the planted redundancy of tests/golden/data/pruner_planted.slp is found and removed,
over Z_p and over Q; on 3x4x7_63_rational_R.slp the windows are those of the rule restated in tests/pruner_lib.py, every
best cost is the C oracle's minimum over the window's own seeds, and every printed replacement computes its window's matrix."""
import os

import pytest

import pruner_lib as pl
from plo_testlib import DATA, FieldP, FieldQ, OracleMatrix, count_ops, eval_slp, oracle_chain

P = 131071
PLANTED = os.path.join(DATA, "pruner_planted.slp")
R347 = os.path.join(DATA, "3x4x7_63_rational_R.slp")


@pytest.fixture(scope="module", autouse=True)
def _build():
    pl.build()


@pytest.mark.parametrize("field", [["-q", str(P)], []], ids=["mod_p", "rationals"])
def test_planted_redundancy_is_reported(field):
    rc, out, err = pl.run(["-v", "--gpu", "0", "-O", "10"] + field + [PLANTED])
    assert rc == 0, err
    wins = pl.report(out)
    assert [w["sel"] for w in wins] == [["t1"], ["t2"]]
    t2 = wins[1]
    assert t2["mark"] == "IMPROVEMENT" and t2["before"] == (3, 0) and t2["dims"] == (2, 3)
    assert min(t2["D"][:2], t2["G"][:2]) == (2, 0) and count_ops("\n".join(t2["repl"])) == (2, 0)
    assert all(w["mark"] != "≤" for w in wins)
    assert "# windows: 2 kept" in err


@pytest.mark.parametrize("field", [["-q", str(P)], []], ids=["mod_p", "rationals"])
@pytest.mark.parametrize("singles", [["-v"], []], ids=["singles", "pairs"])
def test_apply_removes_one_operation_and_keeps_the_matrix(tmp_path, field, singles):
    text = open(PLANTED).read()
    rc, sms, err = pl.run(field + [PLANTED], tool=pl.CHK)
    assert rc == 0, err
    mat = tmp_path / "planted.sms"
    mat.write_text(sms)
    rc, out, err = pl.run(singles + ["--gpu", "0", "-O", "10", "--apply"] + field + [PLANTED])
    assert rc == 0 and "--apply: window" in err, err
    a0, m0 = count_ops(text)
    assert count_ops(out) == (a0 - 1, m0)
    rc, _, err = pl.run(field + ["-M", str(mat)], stdin=out, tool=pl.CHK)
    assert rc == 0 and "SUCCESS" in err, err
    F = FieldP(P) if field else FieldQ
    assert eval_slp(out, F) == eval_slp(text, F)


@pytest.fixture(scope="module")
def singles347():
    rc, out, err = pl.run(["-v", "-q", P, "-O", 20, "--gpu", "0", R347])
    assert rc == 0, err
    return pl.report(out), pl.windows(open(R347).read(), singles=True), err


def test_windows_are_those_of_the_rule(singles347):
    got, want, err = singles347
    assert len(got) == len(want) == 15 and "# windows: 15 kept, 0 skipped" in err
    for g, w in zip(got, want):
        assert g["sel"] == w["sel"] and g["dims"] == (len(w["outs"]), len(w["ins"])) and g["before"] == w["before"], w["sel"]
    assert min(g["dims"] for g in got) == (3, 7) and max(g["dims"] for g in got) == (13, 17)


def test_best_costs_are_the_oracles_minima(singles347):
    got, want, _ = singles347
    N = 20
    for k, (g, w) in enumerate(zip(got, want)):
        m, n = g["dims"]
        O = OracleMatrix(*(pl.csr_of(pl.window_matrix(w, FieldP(P)), m, n) + (P,)))
        assert g["D"] == O.search(k * N, N), w["sel"]
        U, L, _rank = O.lu_factors()
        ch = [oracle_chain(U, L, s) for s in range(k * N, (k + 1) * N)]
        j = min(range(N), key=lambda j: (sum(ch[j]), ch[j][0], j))
        assert g["G"] == ch[j] + (k * N + j,), w["sel"]
        best = min(g["D"][:2], g["G"][:2], key=lambda x: (sum(x), x[0]))
        dif = sum(g["before"]) - sum(best)
        assert g["mark"].split(" ")[0] == ("IMPROVEMENT" if dif > 0 else "==" if dif == 0 else "≤")


def test_every_printed_replacement_computes_its_window(tmp_path):
    """pairs over three variables of a program with a planted second copy of one of its lines, so that replacements exist"""
    text = open(R347).read().replace("g11:=i11-o42;", "g11:=i11-o42;\nz0:=i9+o10;\nz1:=z0+i11;")
    src = tmp_path / "planted347.slp"
    src.write_text(text)
    only = ["g9", "z0", "g11"]
    rc, out, err = pl.run(["-q", P, "-O", 20, "--gpu", "0", "-l", "^(g9|z0|g11)$", str(src)])
    assert rc == 0, err
    got, want = pl.report(out), pl.windows(text, singles=False, only=only)
    assert len(got) == len(want) == 9
    shown = 0
    for g, w in zip(got, want):
        assert g["sel"] == w["sel"] and g["dims"] == (len(w["outs"]), len(w["ins"])) and g["before"] == w["before"]
        if w["sel"][0] != w["sel"][1]:
            assert w["sel"][1] in w["outs"] and w["sel"][0] not in w["outs"]       # the second selected variable stays an output
        assert (g["mark"] == "IMPROVEMENT") == bool(g["repl"])
        if g["repl"]:
            shown += 1
            assert eval_slp(pl.renamed(g["repl"], w), FieldP(P)) == pl.window_matrix(w, FieldP(P)), w["sel"]
            best = min(g["D"][:2], g["G"][:2], key=lambda x: (sum(x), x[0]))
            assert count_ops("\n".join(g["repl"])) == best
            if w["sel"][0] != w["sel"][1]:
                assert any(l.startswith(w["sel"][1] + ":=") for l in g["repl"])
    assert shown >= 4


def test_a_constant_that_is_no_unit_stops_the_tool(tmp_path):
    src = tmp_path / "three.slp"
    src.write_text("t0:=i0*3+i1;\no0:=t0+i2;\no1:=t0/6;\n")
    rc, out, err = pl.run(["-v", "-q", 3, "--gpu", "0", str(src)])
    assert rc != 0 and out == "" and "no unit modulo 3" in err, err
    rc, out, err = pl.run(["-v", "-q", 7, "--gpu", "0", str(src)])
    assert rc == 0 and len(pl.report(out)) == 1, err
