"""bin/growthfactor on the host: its text against the restatement of the reference's src/growthfactor.cpp in
tests/orbit_growth_oracle.py on every fixture triple whose shapes are r x mk, r x kn, mn x r; the G2 that the names of the
reference's data files carry; the statuses."""
import math
import os
import re
import subprocess

import pytest

import orbit_growth_oracle as G
import orbit_oracle as O
from plo_testlib import DATA, ROOT, read_sms

GF = os.path.join(ROOT, "bin", "growthfactor")


def files(name):
    return [os.path.join(DATA, "%s_%s.sms" % (name, x)) for x in "LRP"]


def triples():
    """the names with all three files and shapes of a matrix-multiplication triple"""
    names = sorted({f[:-6] for f in os.listdir(DATA) if f.endswith("_L.sms")})
    out = []
    for nm in names:
        if not all(os.path.exists(f) for f in files(nm)):
            continue
        try:
            shapes = [read_sms(f)[:2] for f in files(nm)]
        except ValueError:                                 # (polynomial coefficients: no rational triple)
            continue
        if O.shape(*shapes):
            out.append(nm)
    return out


TRIPLES = triples()


def run(args):
    r = subprocess.run([GF] + args, capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


def g2_of(name):
    rc, out, err = run(files(name))
    assert rc == 0, err
    return float(re.search(r"^## G2:\t\t(\S+)\t", err, re.M).group(1))


def test_the_fixtures_are_found():
    assert len(TRIPLES) >= 25 and {"2x2x2_7_Winograd", "4x4x4_49_156", "3x4x7_63_rational", "3x6x3_40_DPS-accurate"} <= set(TRIPLES)


@pytest.mark.parametrize("name", TRIPLES)
def test_text_equals_the_oracle(name):
    """fails without the feature: there is no bin/growthfactor"""
    mats, mkn = O.load(os.path.join(DATA, name))
    rc, out, err = run(files(name))
    assert rc == 0 and out == ""
    assert err == G.growthfactor_text(mats, mkn)
    assert len(err.splitlines()) == 13 and len(re.findall(r"^## ", err, re.M)) == 11


@pytest.mark.parametrize("name", ["2x2x2_7_DPS-integral-12.0662", "2x2x2_7_DPS-smallrat-12.2034", "2x2x2_7_DPS-intermediate-12.0695"])
def test_g2_is_the_number_in_the_file_name(name):
    assert "%.4f" % g2_of(name) == name.rsplit("-", 1)[1]


def test_g2_of_strassen_and_the_recorded_table():
    assert "%.4f" % g2_of("2x2x2_7_Strassen") == "%.4f" % (12 + 2 * math.sqrt(2))
    for name, want in [("2x2x2_7_Winograd", "17.8530"), ("4x4x4_49_156", "318.7298"), ("4x4x4_48_accurate", "154.5097"), ("3x3x3_23_58", "83.1646"),
                       ("3x6x3_40_DPS-accurate", "104.0908")]:
        assert "%.4f" % g2_of(name) == want, name


def test_statuses(tmp_path):
    w, t = files("2x2x2_7_Winograd"), files("3x3x3_23_58")
    rc, out, err = run([w[0], t[1], w[2]])                 # 7 rows of L, 23 of R
    assert rc == 2 and "inner dimension mismatch: 7(.)23|7" in err
    rc, out, err = run([w[0], w[1], files("3x3x6_40")[2]])                                         # 40 columns of P
    assert rc == 2 and "inner dimension mismatch: 7(.)7|40" in err
    p = tmp_path / "P.sms"                                 # inner dimensions agree, 4 x 4 x 3 x 7 is no m k, k n, m n
    p.write_text("3 7 R\n1 1 1\n0 0 0\n")
    rc, out, err = run([w[0], w[1], str(p)])
    assert rc == 2 and "are not r x mk, r x kn, mn x r" in err
    for args in (["-h"], w[:2], []):
        rc, out, err = run(args)
        assert rc == 255 and err.startswith("Usage:") and "L.sms R.sms P.sms" in err
