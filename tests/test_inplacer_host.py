"""bin/inplacer on the host (--gpu 0), held to the literal oracle tests/lin_oracle.py and to tests/golden/lin_costs.json;
the reference's own check of the tool (bin/FDT.sh:78,80: `inplacer -O N f | SLPchecker -M f`, and the transposed form fed
with the transpose of f); SLPchecker on programs that read t# inputs; the empty-row barrier; the variant-1 finding."""
import glob
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import pytest

import lin_oracle as O
from plo_testlib import DATA, GOLDEN, ROOT, read_sms

INP = os.path.join(ROOT, "bin", "inplacer")
CHK = os.path.join(ROOT, "bin", "SLPchecker")
GOLD = json.load(open(os.path.join(GOLDEN, "lin_costs.json")))


def run(cmd, stdin=None):
    r = subprocess.run(cmd, input=stdin, capture_output=True, text=True, timeout=300)
    return r.returncode, r.stdout, r.stderr


def sms_text(m, n, ent):
    out = ["%d %d R" % (m, n)]
    for (i, j), v in sorted(ent.items()):
        out.append("%d %d %s" % (i + 1, j + 1, O.fstr(v)))
    return "\n".join(out + ["0 0 0", ""])


def fdt_files():
    return [f for f in sorted(glob.glob(os.path.join(DATA, "*.sms"))) if "-X_" not in f and "32x32x32" not in f]


@pytest.mark.parametrize("name,tr,seed,loops", [("2x2x2_7_Winograd_L", False, 0, 6), ("2x2x2_7_Winograd_R", True, 3, 6),
                                                ("2o2o2_4_partSP_L", True, 1, 5), ("4x4x4_49_156_L", False, 7, 4),
                                                ("3x3x3_23_58_P", True, 11, 4), ("2x2x2_7_DPS-accurate_L", False, 2, 5),
                                                ("4x4x4_48_rational_L", True, 5, 2)])
def test_text_equals_oracle(name, tr, seed, loops):
    """stdout of `inplacer --gpu 0 [-t] --seed s -O n f` == the oracle's FindProgram (src/inplacer.cpp:38-80), byte for byte"""
    f = os.path.join(DATA, name + ".sms")
    rc, out, err = run([INP, "--gpu", "0", "--seed", str(seed), "-O", str(loops), f] + (["-t"] if tr else []))
    assert rc == 0, err
    m, n, e = read_sms(f)
    want, ops = O.find_program(m, n, e, tr, seed, loops)
    assert out == want
    assert "# \033[1;32m%d\tADD\033[0m\n# \033[1;32m%d\tSCA\033[0m\n# \033[1;32m%d\tROWS\033[0m" % ops in err


def test_host_counts_equal_golden():
    """per-seed (ADD, SCA, ROWS) of both variants on the host == lin_costs.json, every fixture direct and transposed"""
    seeds = GOLD["seeds"]
    assert seeds == list(range(len(seeds)))

    def one(key):
        name, how = key.split("|")
        rc, out, err = run([INP, "--gpu", "0", "--costs", "-O", str(len(seeds)), os.path.join(DATA, name + ".sms")] + (["-t"] if how == "t" else []))
        assert rc == 0, err
        got = [[int(x) for x in line.split()[1:]] for line in out.splitlines()]
        return key, got

    assert len(GOLD["fixtures"]) >= 280
    with ThreadPoolExecutor(max_workers=8) as ex:
        for key, got in ex.map(one, sorted(GOLD["fixtures"])):
            assert got == GOLD["fixtures"][key], key


def test_host_counts_equal_golden_long_run():
    L = GOLD["long"]
    rc, out, err = run([INP, "--gpu", "0", "--costs", "--seed", str(L["seed0"]), "-O", str(L["n"]), os.path.join(DATA, L["name"] + ".sms")])
    assert rc == 0, err
    lines = out.splitlines()
    assert [int(x) for x in lines[0].split()[1:4]] == L["base"][:3]
    got = [int(x) for line in lines[1:] for x in line.split()[1:]]
    assert got == L["ops"]


@pytest.mark.parametrize("transposed", [False, True])
def test_fdt_inplacer_lines(transposed, tmp_path):
    """bin/FDT.sh:78 `inplacer -O 10 f | SLPchecker -M f` and :80 `matrix-transpose f | inplacer -t -O 10 | SLPchecker -M f`
    print SUCCESS on every data matrix FDT takes (no -X_ placeholders, no 32x32x32)"""
    files = fdt_files()
    assert len(files) >= 140

    def one(f):
        if transposed:
            m, n, e = read_sms(f)
            rc, prog, err = run([INP, "--gpu", "0", "-t", "-O", "10"], stdin=sms_text(*O.transpose(m, n, e)))
        else:
            rc, prog, err = run([INP, "--gpu", "0", "-O", "10", f])
        assert rc == 0, (f, err)
        rc, _, e2 = run([CHK, "-M", f], stdin=prog)
        assert rc == 0 and "SUCCESS" in e2, (f, e2)

    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(one, files))


def test_several_files_in_order_and_stdin():
    """several files one after another (src/inplacer.cpp:136-141); stdin without a file"""
    a, b = os.path.join(DATA, "2x2x2_7_Winograd_L.sms"), os.path.join(DATA, "2o2o2_4_partSP_L.sms")
    rc, both, _ = run([INP, "--gpu", "0", "-O", "3", a, b])
    rc1, oa, _ = run([INP, "--gpu", "0", "-O", "3", a])
    rc2, ob, _ = run([INP, "--gpu", "0", "-O", "3"], stdin=open(b).read())
    assert rc == rc1 == rc2 == 0 and both == oa + ob


def test_slpchecker_reads_letter_inputs():
    """an unassigned <letter><index> is input column <index> (matrixBuilder, plinopt_programs.inl:1517-1524); other
    undefined words still fail"""
    sms = "2 3 R\n1 1 1\n1 3 -2\n2 2 1/3\n0 0 0\n"
    prog = "z0:=t0;\nz1:=t1;\nz2:=t2;\no0:=z0-z2*2;\no1:=z1/3;\n"
    rc, out, err = run([CHK], stdin=prog)
    assert rc == 0 and out == sms, (out, err)
    rc, out_i, _ = run([CHK], stdin=prog.replace("t", "i"))
    assert rc == 0 and out_i == out
    rc, _, err = run([CHK], stdin="o0:=tmp+t1;\n")
    assert rc != 0 and "undefined variable tmp" in err


def test_empty_row_barrier_stops_walks_by_position():
    """an empty row l is the barrier Atom(' ', l, ' ', 0) (:474-476); simplify's stop rule compares _src only (:287-293), so a
    walk of an atom on z_l stops there.  Rows 0 and 2 are the same and row 1 is empty: with pivot column 1 the undo of row 0
    and the redo of row 2 do NOT cancel (ADD 4), with pivot column 2 they do (ADD 2)."""
    m, n, e = 3, 3, {k: Fraction(1) for k in [(0, 1), (0, 2), (2, 1), (2, 2)]}
    rows = O.rows_of(m, n, e)
    seen = set()
    for s in [O.BASE_SEED] + list(range(400)):
        perm, v = O.candidate(rows, n, s)
        if perm[1] == 1:
            prog = v[0][1]
            piv = {a.src for a in prog if a.ope == " " and a.var == "z"}
            if len(piv) == 1:
                seen.add((piv.pop(), v[0][0][0]))
    assert (1, 4) in seen and (2, 2) in seen, seen
    text = sms_text(m, n, e)
    rc, out, err = run([INP, "--gpu", "0", "--costs", "-O", "400"], stdin=text)
    assert rc == 0, err
    got = [[int(x) for x in line.split()[1:]] for line in out.splitlines()]
    assert got == [O.cost6(rows, n, s) for s in [O.BASE_SEED] + list(range(400))]
    rc, prog, _ = run([INP, "--gpu", "0", "-O", "40"], stdin=text)
    assert rc == 0 and prog.count(":=0;") == 1


def test_empty_row_program_checks(tmp_path):
    m, n, e = read_sms(os.path.join(DATA, "2o2o2_4_partSP_L.sms"))
    f = tmp_path / "T.sms"
    f.write_text(sms_text(*O.transpose(m, n, e)))
    for seed in range(5):
        rc, prog, err = run([INP, "--gpu", "0", "--seed", str(seed), "-O", "4", str(f)])
        assert rc == 0, err
        assert prog.count(":=0;") == 1
        rc, _, e2 = run([CHK, "-M", str(f)], stdin=prog)
        assert rc == 0 and "SUCCESS" in e2, e2


def test_variant1_finding_and_printing(tmp_path):
    """over every fixture candidate of lin_costs.json and 10^4 seeds on 4x4x4_49_156_L, the appended
    variant never beats the incumbent (:613) nor variant 0 of its own seed.  Should it win, its 2m barriers print as outputs
    perm[k mod m] (the reference reads past the permutation): each output is assigned the same value twice, and the program
    passes SLPchecker -M.  --candidate s 1 prints that text."""
    v1 = GOLD["variant1"]
    assert v1["fixture_candidates"] >= 2000 and v1["beats_incumbent"] == 0 and v1["beats_variant0"] == 0
    assert GOLD["long"]["n"] >= 10000 and v1["long_beats_incumbent"] == 0 and v1["long_beats_variant0"] == 0
    ops = GOLD["long"]["ops"]
    assert all((ops[6 * k + 3], ops[6 * k + 4]) > (ops[6 * k], ops[6 * k + 1]) for k in range(len(ops) // 6))
    for name, tr, seed in [("2x2x2_7_Winograd_L", False, 4), ("2o2o2_4_partSP_L", True, 2), ("4x4x4_48_rational_P", False, 1)]:
        f = os.path.join(DATA, name + ".sms")
        m, n, e = read_sms(f)
        rc, prog, err = run([INP, "--candidate", str(seed), "1", f] + (["-t"] if tr else []))
        assert rc == 0, err
        mm, nn, ee = O.transpose(m, n, e) if tr else (m, n, e)
        perm, v = O.candidate(O.rows_of(mm, nn, ee), nn, seed)
        want = O.input2temps(m if tr else n, "t" if tr else "i", "z") + O.pprint("o", v[1][1], perm)
        assert prog == want
        assert v[1][0][2] == 2 * mm and sum(1 for line in prog.splitlines() if line.startswith("o")) == 2 * mm
        if tr:
            g = tmp_path / "T.sms"
            g.write_text(sms_text(*O.transpose(m, n, e)))
            rc, _, e2 = run([CHK, "-M", str(g)], stdin=prog)
        else:
            rc, _, e2 = run([CHK, "-M", f], stdin=prog)
        assert rc == 0 and "SUCCESS" in e2, e2


def test_without_device_no_silent_fallback():
    """the default is the device: without one the tool fails (--gpu 0 selects the host loop), as bin/trilplacer"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rc, out, err = run([INP, "-O", "5", os.path.join(DATA, "2x2x2_7_Winograd_L.sms")])
    assert rc == 2 and out == "" and "no CPU fallback" in err
