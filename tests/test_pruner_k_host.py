"""bin/pruner -K on the host (--gpu 0): the K group stands exactly at the windows whose matrix has a kernel, with the C oracle's
minimum of plo_oracle_kernel_restart over the window's own seeds; the mark is that of the best of D, K and G; replacements
that the kernel method wins compute their window, define every variable once and count what the search counted; --apply
keeps the program's matrix; over Q the replacements compute their windows; and without -K the tool prints what it printed
before (tests/golden/pruner_3x4x7_R_O20.txt, from the build before -K existed)."""
import os

import pytest

import pruner_k_lib as kl
from plo_testlib import DATA, GOLDEN, FieldP, FieldQ, OracleMatrix, count_ops, eval_slp

P = 131071
R347 = os.path.join(DATA, "3x4x7_63_rational_R.slp")
L347 = os.path.join(DATA, "3x4x7_63_rational_L.slp")
PLANTED = os.path.join(DATA, "pruner_planted.slp")
# Window t2 is [t1; t0; o2] = three dense rows of which the third is the sum of the other two, with coefficients that share no ratio:
# Optimizer finds nothing to share (9|9), the LU chain pays for the rows of U (7|7), the kernel method adds two outputs (7|6).
# (A DUPLICATED dense row would not do: Optimizer shares every pair of it and ties with the kernel method, and ties go to D.)
KWIN = "t0:=i0+i1*2+i2*3+i3*5;\nt1:=i0-i1*3+i2*7-i3*2;\nt2:=i0*2-i1+i2*10+i3*3;\no0:=t0+i4;\no1:=t1-i4;\no2:=t2;\n"


@pytest.fixture(scope="module", autouse=True)
def _build():
    kl.pl.build()


def oracle_of(w, p=P):
    m, n = len(w["outs"]), len(w["ins"])
    return OracleMatrix(*(kl.csr_of(kl.window_matrix(w, FieldP(p)), m, n) + (p,)))


def test_k_group_is_the_oracles_minimum_where_there_is_a_kernel():
    N = 20
    rc, out, err = kl.run(["-q", P, "-K", "-O", N, "--gpu", "0", R347])
    assert rc == 0, err
    got, want = kl.report(out), kl.windows(open(R347).read(), singles=False)
    assert len(got) == len(want) == 225
    withk = 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["sel"] == w["sel"] and g["D"] is None and g["G"] is None
        exp = kl.kernel_min(oracle_of(w), k * N, N)
        assert g["K"] == exp, (w["sel"], g["K"], exp)
        if exp:
            withk += 1
            assert g["mark"].split(" ")[0] == kl.mark_of(g), w["sel"]
    assert withk == 118


def test_every_window_of_an_l_program_has_a_k_group():
    rc, out, err = kl.run(["-q", P, "-K", "-O", 20, "--gpu", "0", "-l", "^(t26|b76|e1)$", L347])
    assert rc == 0, err
    got, want = kl.report(out), kl.windows(open(L347).read(), singles=False, only=["t26", "b76", "e1"])
    assert len(got) == len(want) == 9
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["K"] is not None and g["K"] == kl.kernel_min(oracle_of(w), k * 20, 20), w["sel"]


def check_replacements(text, args, field, min_shown, singles=False, only=None):
    got, want = kl.report(args), kl.windows(text, singles=singles, only=only)
    assert len(got) == len(want)
    shown, byk = 0, 0
    for g, w in zip(got, want):
        assert g["sel"] == w["sel"] and (g["mark"] == "IMPROVEMENT") == bool(g["repl"])
        assert g["mark"].split(" ")[0] == kl.mark_of(g), w["sel"]
        if g["repl"]:
            shown += 1
            method, best = kl.best_of(g)
            byk += method == "K"
            assert eval_slp(kl.renamed(g["repl"], w), field) == kl.window_matrix(w, field), w["sel"]
            assert kl.defined_once(g["repl"]), g["repl"]
            assert count_ops("\n".join(g["repl"])) == best, w["sel"]
    assert shown >= min_shown
    return byk


def test_every_printed_replacement_computes_its_window(tmp_path):
    """the planted copy of tests/test_pruner_host.py with all three methods (the kernel method only ties there), and KWIN, whose
    window t2 the kernel method wins"""
    text = open(R347).read().replace("g11:=i11-o42;", "g11:=i11-o42;\nz0:=i9+o10;\nz1:=z0+i11;")
    src = tmp_path / "planted347.slp"
    src.write_text(text)
    rc, out, err = kl.run(["-q", P, "-O", 20, "--gpu", "0", "-D", "-K", "-G", "-l", "^(g9|z0|g11)$", str(src)])
    assert rc == 0, err
    byk = check_replacements(text, out, FieldP(P), 4, only=["g9", "z0", "g11"])
    assert sum(1 for g in kl.report(out) if g["K"]) >= 6
    src2 = tmp_path / "kwin.slp"
    src2.write_text(KWIN)
    rc, out, err = kl.run(["-q", P, "-v", "-O", 20, "--gpu", "0", "-D", "-K", "-G", str(src2)])
    assert rc == 0, err
    byk += check_replacements(KWIN, out, FieldP(P), 3, singles=True)
    t2 = kl.report(out)[2]
    assert t2["sel"] == ["t2"] and kl.best_of(t2)[0] == "K" and byk >= 1


@pytest.mark.parametrize("text", [KWIN, None], ids=["kwin", "planted"])
def test_apply_with_k_keeps_the_matrix(tmp_path, text):
    text = text or open(PLANTED).read()
    src = tmp_path / "in.slp"
    src.write_text(text)
    rc, sms, err = kl.run(["-q", P, str(src)], tool=kl.pl.CHK)
    assert rc == 0, err
    mat = tmp_path / "in.sms"
    mat.write_text(sms)
    rc, out, err = kl.run(["-v", "--gpu", "0", "-O", 10, "--apply", "-K", "-q", P, str(src)])
    assert rc == 0, err
    rc, _, err2 = kl.run(["-q", P, "-M", str(mat)], stdin=out, tool=kl.pl.CHK)
    assert rc == 0 and "SUCCESS" in err2, err2
    if text == KWIN:
        assert "--apply: window t2" in err and sum(count_ops(out)) < sum(count_ops(text))


def test_over_the_rationals_replacements_compute_their_windows(tmp_path):
    src = tmp_path / "kwin.slp"
    src.write_text(KWIN)
    rc, out, err = kl.run(["-K", "-v", "-O", 10, "--gpu", "0", str(src)])
    assert rc == 0, err
    got, want = kl.report(out), kl.windows(KWIN, singles=True)
    assert [g["sel"] for g in got] == [w["sel"] for w in want] and got[2]["K"] and got[2]["repl"]
    rc, out2, err = kl.run(["-K", "-v", "-O", 5, "--gpu", "0", R347])
    assert rc == 0, err
    for g, w in list(zip(got, want)) + list(zip(kl.report(out2), kl.windows(open(R347).read(), singles=True))):
        assert g["sel"] == w["sel"]
        if g["repl"]:
            assert eval_slp(kl.renamed(g["repl"], w), FieldQ) == kl.window_matrix(w, FieldQ), w["sel"]


def test_without_k_the_output_is_what_it_was():
    rc, out, err = kl.run(["-q", P, "-O", 20, "--gpu", "0", R347])
    assert rc == 0, err
    assert out == open(os.path.join(GOLDEN, "pruner_3x4x7_R_O20.txt")).read()
    rc, _, err = kl.run(["-h"])
    assert rc == 0 and "[-K]" in err and "-D -K -G" in err
