"""bin/PMchecker --gpu 0: the host loop over every coefficient equation, its verdicts on the fixture triples against the
independent oracle of tests/polymul_lib.py, the parser of -P, the exit statuses, and the certificate over Q.  No GPU."""
import os
import re
import subprocess
from fractions import Fraction

import pytest

import polymul_lib as M
from plo_testlib import ROOT

PMC = os.path.join(ROOT, "bin", "PMchecker")
ANSI = re.compile(r"\x1b\[[0-9;]*m")


def pmc(args, gpu=0, timeout=120):
    r = subprocess.run([PMC, "--gpu", str(gpu)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    return r.returncode, ANSI.sub("", r.stderr)


def options(q, f, X="X"):
    return (["-q", q] if q else []) + (["-P", M.poly_text(f, X)] + (["-I", X] if X != "X" else []) if f else [])


def first_of(err):
    """(e, (i, j, c), found text, expected text) of the `# first violated equation` line"""
    mt = re.search(r"# first violated equation e=(\d+): \(i,j,c\) = \((\d+),(\d+),(\d+)\), found (\S+) instead of ([^\s;]+)", err)
    assert mt, err
    return int(mt.group(1)), tuple(int(mt.group(k)) for k in (2, 3, 4)), mt.group(5), mt.group(6)


def cert_of(err):
    mt = re.search(r"# certificate: beta = (\d+), j = (\d+), primes((?: \d+)+)", err)
    assert mt, err
    return int(mt.group(1)), int(mt.group(2)), [int(x) for x in mt.group(3).split()]


def passes_of(err):
    return [(int(a), int(b), int(p), t) for a, b, p, t in re.findall(r"# pass (\d+) of (\d+) modulo (\d+): (no violated equation|violated)", err)]


def field(q):
    return "Z/%dZ" % q if q else "Q"


def shape_text(T):
    na, nb, nc, _ = M.shape(T)
    return "%do%do%d" % (na - 1, nb - 1, nc - 1)


def test_the_four_pmcheck_lines():
    """the reference's `make pmcheck`, options behind the files as it writes them"""
    for name, opts in (("4o4o8_Toom5", []), ("4o4o8_Montgomery-13", []), ("4o4o4_F243-11-44", ["-q", "3", "-P", "1-X+X^5"]),
                       ("4o4o4_F243-Montgomery-13-42", ["-q", "3", "-P", "X^5+X^4-X^3-X^2-1"])):
        rc, err = pmc(M.files(name) + opts)
        assert rc == 0 and "# SUCCESS: correct %s Polynomial-Multiplication over %s" % (name[:5], "Z/3Z" if opts else "Q") in err, err
        assert ("# host: " in err) and "# GPU:" not in err


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_fixture_verdicts(case):
    name, q, f, count = case
    T = M.load(name)
    want = M.oracle(T, q, f)
    assert want[0] == count
    rc, err = pmc(options(q, f) + ["--count"] + M.files(name))
    w = M.width(T, f)
    if count == 0:
        assert rc == 0, err
        line = [ln for ln in err.splitlines() if "SUCCESS" in ln]
        assert len(line) == 1 and line[0].startswith("# SUCCESS: correct %s Polynomial-Multiplication over %s " % (shape_text(T), field(q))), err
        assert ("mod " in line[0]) == bool(f) and "ERROR" not in err
    else:
        assert rc == 1, err
        assert "****** ERROR, not a %s MM algorithm over %s******" % (shape_text(T), field(q)) in err and "SUCCESS" not in err
        e, ijc, got, exp = first_of(err)
        pair, c = divmod(want[1], w)
        assert (e, ijc) == (want[1], divmod(pair, T[1][1]) + (c,))
        assert (got, exp) == (str(want[2]), str(want[3]))
        assert "# %d of %d equations violated" % (count, T[0][1] * T[1][1] * w) in err
        rc2, err2 = pmc(options(q, f) + M.files(name))                                  # without --count: the same first equation
        assert rc2 == 1 and first_of(err2) == (e, ijc, got, exp) and "equations violated" not in err2
    if q == 0:
        beta, j = M.certificate(T, f)
        gb, gj, primes = cert_of(err)
        assert (gb, gj) == (beta, j) and primes[0] == M.P31 and len(primes) == j
        assert beta >= M.cleared_defect_bits(T, f)


@pytest.mark.parametrize("text,X,f", [
    ("1-X+X^5", "X", "1 -1 0 0 0 1"), ("X^5 + X^4 - X^3 - X^2 - 1", "X", "-1 0 -1 -1 1 1"), (" 1 - X + X ^ 5 ", "X", "1 -1 0 0 0 1"),
    ("-2/3*X^2+1/2", "X", "1/2 0 -2/3"), ("- 2 / 3 X^2 + 1/2", "X", "1/2 0 -2/3"), ("X^3", "X", "0 0 0 1"), ("1-y+y^5", "y", "1 -1 0 0 0 1"),
    ("X^5+1-3*X+2X+X^5-X^5", "X", "1 -1 0 0 0 1"), ("+X^5-X^1+X^0", "X", "1 -1 0 0 0 1"), ("2*X^5-2*X+2", "X", "1 -1 0 0 0 1"),
])
def test_the_parser_in_the_tool(tmp_path, text, X, f):
    f = M.poly(f)
    files = M.write_triple(tmp_path, M.schoolbook_folded(3, 4, f))
    rc, err = pmc(["-P", text] + (["-I", X] if X != "X" else []) + files)
    assert rc == 0 and "SUCCESS" in err, err
    other = "X^5+X^4-X^3-X^2-1" if "X^5 + X^4" not in text else "1-X+X^5"               # another polynomial of degree 5: the verdict depends on what was read
    if len(f) == 6:
        rc, err = pmc(["-P", other] + files)
        assert rc == 1, err


@pytest.mark.parametrize("text", ["", " ", "X^", "1-*X", "2**X", "1-Y", "X^5-", "1/0*X", "X X", "1 2", "(X+1)", "X^-2", "1/X", "x^2+1", "3*", "X^2^3", "1.5*X"])
def test_unparsable_polynomials_are_refused(text):
    rc, err = pmc(["-P", text] + M.files("4o4o8_Toom5"))
    assert rc == 4 and "ERROR" in err and "SUCCESS" not in err, (text, err)


def test_exit_statuses(tmp_path):
    F = M.files("4o4o4_F243-11-44")
    T = M.load("4o4o4_F243-11-44")
    for text in ("7", "3/2", "X-X+1", "0*X^3+2"):                                     # a constant
        rc, err = pmc(["-q", 3, "-P", text] + F)
        assert rc == 4 and "constant" in err, err
    rc, err = pmc([F[0], M.files("4o4o8_Toom5")[1], F[2]])
    assert rc == 2 and "****** ERROR, inner dimension mismatch: 11(.)9|11 ******" in err, err
    rc, err = pmc(["-q", 3, "-P", "1-X+3*X^5"] + F)                                   # a leading coefficient that is no unit
    assert rc == 4 and "leading coefficient" in err and "not invertible modulo 3" in err
    rc, err = pmc(["-q", 6, "-P", "1-X+2*X^5"] + F)
    assert rc == 4 and "leading coefficient" in err
    rc, err = pmc(["-q", 3, "-P", "1/3-X+X^5"] + F)                                   # a denominator of f
    assert rc == 4 and "not invertible modulo 3" in err
    third = M.write_triple(tmp_path, M.changed(T, 0, 0, 0, Fraction(1, 3)))            # and one of a matrix
    rc, err = pmc(["-q", 3, "-P", "1-X+X^5"] + third)
    assert rc == 4 and "not invertible modulo 3" in err
    rc, err = pmc(["-q", 1] + F)
    assert rc == 4
    rc, err = pmc([F[0], F[1], str(tmp_path / "missing.sms")])
    assert rc == 4 and "cannot read" in err
    rc, err = pmc(["-I", "XY", "-P", "1-X+X^5"] + F)
    assert rc == 4
    rc, err = pmc(["--pairs", "20:6", "-q", 3, "-P", "1-X+X^5"] + F)
    assert rc == 4 and "--pairs" in err
    rc, err = pmc(["-b", 12, "-q", 3, "-P", "1-X+X^5"] + F)                           # accepted, no effect
    assert rc == 0 and "SUCCESS" in err
    rc, err = pmc(["-h"])
    assert "no randomness" in err and "-P" in err
    rc, err = pmc(["-q", 2 ** 40 + 15] + M.files("4o4o8_Montgomery-13"))               # the 62-bit field of the host
    assert rc == 0 and "over Z/%dZ" % (2 ** 40 + 15) in err
    rc, err = pmc(["-q", 4, "-P", "1+X^2+X^5"] + M.files("4o4o4_F32_Standard"))       # -q is taken as given: 4 stays 4
    assert "over Z/4Z" in err and rc == (0 if M.oracle(M.load("4o4o4_F32_Standard"), 4, M.F32S)[0] == 0 else 1)


def test_mmchecker_still_refuses_polynomials():
    r = subprocess.run([os.path.join(ROOT, "bin", "MMchecker"), "--gpu", "0", "-P", "X^3"] + M.files("2o2o2_5_shortproduct"), capture_output=True, text=True, timeout=60)
    assert r.returncode == 4 and "polynomial quotients (-P) are not supported" in r.stderr


def test_pair_ranges_compose(tmp_path):
    name, q, f = "4o4o4_S243_10-43", 3, M.F243
    T = M.load(name)
    full = M.oracle(T, q, f)
    npairs, w = 25, 5
    cut = full[1] // w + 1                                                            # the first violated pair ends the first range
    counts = []
    for p0, cnt in ((0, cut), (cut, npairs - cut), (cut - 1, 1)):
        want = M.oracle(T, q, f, p0, p0 + cnt)
        rc, err = pmc(options(q, f) + ["--count", "--pairs", "%d:%d" % (p0, cnt)] + M.files(name))
        assert "[partial: pairs %d .. %d of %d]" % (p0, p0 + cnt - 1, npairs) in err
        assert rc == 1 and first_of(err)[0] == want[1] and "# %d of %d equations violated" % (want[0], cnt * w) in err
        counts.append(want[0])
    assert counts[0] + counts[1] == full[0]
    rc, err = pmc(options(q, f) + ["--pairs", "0:%d" % (cut - 1)] + M.files(name))
    assert rc == 0 and "SUCCESS" in err and "[partial: pairs 0 .. %d of 25]" % (cut - 2) in err


@pytest.mark.parametrize("f", [None, M.F243], ids=["plain", "folded"])
@pytest.mark.parametrize("primes_in_delta", [1, 2])
def test_certificate_soundness(tmp_path, f, primes_in_delta):
    """A correct triple over Q with one entry of P moved by the first certificate prime, or by the product of the first two:
    right modulo those primes, wrong over Q.  The certificate asks for more primes than divide the change, the passes modulo
    those succeed, a later one fails, and the verdict is the oracle's over Q."""
    T0 = M.load("4o4o8_Toom5")
    assert M.oracle(T0, 0, f)[0] == 0
    _, _, primes0 = cert_of(pmc(options(0, f) + M.files("4o4o8_Toom5"))[1])
    delta = primes0[0] * (primes0[1] if primes_in_delta == 2 else 1)
    assert delta < 2 ** 63
    (z, t), v = [x for x in sorted(T0[2][2].items()) if x[1].denominator == 1][1]           # an integer entry: the changed one fits 64 bits too
    T = M.changed(T0, 2, z, t, v + delta)
    want = M.oracle(T, 0, f)
    assert want[0] > 0
    for p in primes0[:primes_in_delta]:
        assert M.oracle(T, p, f)[0] == 0
    rc, err = pmc(options(0, f) + M.write_triple(tmp_path, T))
    beta, j, primes = cert_of(err)
    assert (beta, j) == M.certificate(T, f) and j > primes_in_delta and beta >= M.cleared_defect_bits(T, f)
    assert primes[:primes_in_delta] == primes0[:primes_in_delta] and all(pow(2, p - 1, p) == 1 for p in primes)
    assert rc == 1 and "****** ERROR, not a 4o4o8 MM algorithm over Q******" in err, err
    ps = passes_of(err)
    assert [x[3] for x in ps] == ["no violated equation"] * primes_in_delta + ["violated"]
    assert [x[2] for x in ps] == primes[:primes_in_delta + 1]
    failing = primes[primes_in_delta]
    wm = M.oracle(T, failing, f)
    e, _, got, exp = first_of(err)
    assert e == wm[1] and "modulo %d: %d instead of %d" % (failing, wm[2], wm[3]) in err
    if e == want[1]:                                                                   # the rational values, where the first equation over Q is that one
        assert (got, exp) == (str(want[2]), str(want[3]))
    for p in primes0[:primes_in_delta]:                                                # each of those primes alone passes
        rc, err = pmc(options(p, f) + M.write_triple(tmp_path, T))
        assert rc == 0 and "SUCCESS" in err


def test_certificate_avoids_the_leading_coefficient_and_denominators(tmp_path):
    """f = 1 + 2147483629 X^2 and an entry with the next prime as its denominator: both primes are passed over"""
    p2 = 2147483587
    f = [Fraction(1), Fraction(0), Fraction(M.P31)]
    T = M.schoolbook(2, 2)                                                            # (no entry has the first prime as its denominator)
    T = M.scaled(T, [Fraction(1), Fraction(p2), Fraction(1), Fraction(1)])
    assert M.oracle(T, 0, f)[0] == 0
    rc, err = pmc(options(0, f) + M.write_triple(tmp_path, T))
    beta, j, primes = cert_of(err)
    assert rc == 0 and "SUCCESS" in err, err
    assert M.P31 not in primes and p2 not in primes and primes[0] == 2147483579 and (beta, j) == M.certificate(T, f)
    assert beta >= M.cleared_defect_bits(T, f)


def test_generated_triples(tmp_path):
    import random
    rng = random.Random(11)
    T = M.karatsuba(3)
    T = M.with_cancelling_pair(M.with_null_products(T, 65, 2, 5, rng), 9, 1, 1, rng)
    for q, f in ((0, None), (2, None), (0, M.F243), (M.P31, M.poly("1 1 0 0 0 0 0 0 0 0 0 0 0 0 1")), (7, M.poly("3 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 1"))):
        assert M.oracle(T, q, f)[0] == 0
        rc, err = pmc(options(q, f) + M.write_triple(tmp_path, T))
        assert rc == 0 and "SUCCESS: correct 7o7o14" in err, err
    B = M.changed(T, 1, 3, 0, 5)
    want = M.oracle(B, 131071, M.F243)
    rc, err = pmc(options(131071, M.F243) + ["--count"] + M.write_triple(tmp_path, B))
    assert rc == 1 and first_of(err)[0] == want[1] and first_of(err)[2:] == (str(want[2]), str(want[3])) and "# %d of 320 equations violated" % want[0] in err
