"""bin/MMchecker --gpu 0: the host loop over every Brent equation, its verdicts on the fixture triples, the first violated
equation and the counts against the independent oracle of tests/brent_lib.py, the certificate line over Q, partial checks
and the refusals.  No GPU.

The fixtures named -ALT and -CoB are a sparsifier's alternative-basis factors and change-of-basis matrices, not triples in
the standard basis: they are no multiplication algorithms (the oracle agrees where their shapes fit at all) and are pinned
with the status they get."""
import glob
import os
import re
import subprocess

import pytest

import brent_lib as B
import orbit_oracle
from plo_testlib import DATA, ROOT

MMC = os.path.join(ROOT, "bin", "MMchecker")
ANSI = re.compile(r"\x1b\[[0-9;]*m")

NAMES = sorted(os.path.basename(f)[:-6] for f in glob.glob(os.path.join(DATA, "*_L.sms")))
MM = [x for x in NAMES if re.match(r"\d+x\d+x\d+_", x)]                      # (the T shapes have no third 'x')
TRIPLES = [x for x in MM if not x.endswith(("-X", "-ALT", "-CoB"))]
NOT_TRIPLES = {"2x2x2_7_DPS-accurate-ALT": 1, "2x2x2_7_DPS-accurate-CoB": 1, "3x4x7_63_rational-ALT": 3, "3x4x7_63_rational-CoB": 1,
               "4x4x4_48_accurate-ALT": 3, "4x4x4_48_accurate-CoB": 1, "4x4x4_48_rational-ALT": 3, "4x4x4_48_rational-CoB": 1}
POLY = {"1o1o2_3_Karatsuba": 3, "2o2o2_4_partSP": 3, "2o2o2_5_shortproduct": 3, "2o2o4_5_Toom3": 3, "2o2o4_Toom3": 3, "3o3o3_F81-Karatsuba-9-21": 1,
        "3o3o3_S81_8_22": 1, "3o3o6_Toom4": 3, "4o4o4_F243-11-44": 3, "4o4o4_F243-Montgomery-13-42": 3, "4o4o4_F32_Montgomery": 3, "4o4o4_F32_Standard": 3,
        "4o4o4_S243_10-43": 3, "4o4o4_S32_13_#2": 3, "4o4o8_Montgomery-13": 3, "4o4o8_Toom5": 3}


def files(name):
    return [os.path.join(DATA, "%s_%s.sms" % (name, x)) for x in "LRP"]


def mmc(args, timeout=120):
    r = subprocess.run([MMC, "--gpu", "0"] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    return r.returncode, ANSI.sub("", r.stderr)


def verdict(err):
    return [ln for ln in err.splitlines() if "SUCCESS" in ln or "ERROR" in ln]


def first_of(err):
    """(e, six indices, sum text, expected) of the `# first violated equation` line"""
    mt = re.search(r"# first violated equation e=(\d+): \(a,b \| b',c \| a',c'\) = \((\d+),(\d+) \| (\d+),(\d+) \| (\d+),(\d+)\), sum (\S+) instead of ([01])", err)
    assert mt, err
    return int(mt.group(1)), tuple(int(mt.group(i)) for i in range(2, 8)), mt.group(8).rstrip(";"), int(mt.group(9))


def cert_of(err):
    mt = re.search(r"# certificate: beta = (\d+), j = (\d+), primes((?: \d+)+)", err)
    assert mt, err
    return int(mt.group(1)), int(mt.group(2)), [int(x) for x in mt.group(3).split()]


def dense_of(T):
    return [orbit_oracle.dense(*M) for M in T[:3]]


def test_the_oracle_agrees_with_the_orbiter_tests_oracle(tmp_path):
    """tests/brent_lib.py's sums against tests/orbit_oracle.py::mm_check, which shares no code with it: on Winograd and on copies
    with one entry changed, over Q and modulo a prime, no violation exactly when mm_check says True; and the tool says the same"""
    W = B.load("2x2x2_7_Winograd")
    (t, x), v = sorted(W[0][2].items())[3]
    (z, t2), v2 = sorted(W[2][2].items())[-1]
    cases = [(W, True), (B.changed(W, 0, t, x, v + 1), False), (B.changed(W, 2, z, t2, 0), False), (B.changed(W, 1, 6, 0, B.Fraction(1, 3)), False)]
    for i, (T, good) in enumerate(cases):
        assert orbit_oracle.mm_check(*dense_of(T), T[3]) is good
        assert (B.oracle_q(T)[0] == 0) is good
        for q in (B.P31, 131071, 7):
            mod = orbit_oracle.mm_check(*dense_of(T), T[3], modulus=q)
            assert (B.oracle_mod(T, q)[0] == 0) is mod
            assert mod or not good
            rc, err = mmc(["-q", q] + B.write_triple(tmp_path, T, stem="c%d" % i))
            assert rc == (0 if mod else 1), err
        rc, err = mmc(B.write_triple(tmp_path, T, stem="c%d" % i))
        assert rc == (0 if good else 1), err
    N = B.changed(W, 0, t, x, v + 7)                                            # wrong over Q and modulo the primes, right modulo 7
    assert not orbit_oracle.mm_check(*dense_of(N), N[3]) and B.oracle_q(N)[0] > 0
    assert orbit_oracle.mm_check(*dense_of(N), N[3], modulus=7) and B.oracle_mod(N, 7)[0] == 0
    assert not orbit_oracle.mm_check(*dense_of(N), N[3], modulus=B.P31) and B.oracle_mod(N, B.P31)[0] > 0
    # m != k != n: a swapped index would show
    T = B.load("3x4x7_63_rational")
    assert orbit_oracle.mm_check(*dense_of(T), T[3], modulus=131071) and B.oracle_mod(T, 131071)[0] == 0


@pytest.mark.parametrize("name", TRIPLES)
def test_fixture_triples_are_correct(name):
    T = B.load(name)
    m, k, n = T[3]
    if name == "2x2x2_7_DPS-accurate":                                       # it holds sqrt(3) as 1013: right modulo 1013^2 - 3 without its factor 2
        q = (1013 ** 2 - 3) // 2
        assert B.oracle_mod(T, q)[0] == 0 and B.oracle_q(T)[0] > 0
        rc, err = mmc(files(name))
        assert rc == 1 and "ERROR, not a 2x2x2 MM algorithm over Q" in err
        rc, err = mmc(["-r", 1013, 2, 3] + files(name))
        field = "Z/%dZ" % q
    else:
        assert B.oracle_mod(T, B.P31)[0] == 0
        rc, err = mmc(files(name))
        field = "Q"
    assert rc == 0, err
    mt = re.search(r"# SUCCESS: correct %dx%dx%d \((\d+),(\d+)\) Matrix-Multiplication over %s" % (m, k, n, re.escape(field)), err)
    assert mt, err
    assert int(mt.group(1)) == sum(len(M[2]) for M in T[:3])
    # the reference's rotater.sh reads the shape off that line
    line = [ln for ln in err.splitlines() if "SUCCESS" in ln][0]
    assert line.replace("x", " ").split(" ")[3:6] == [str(m), str(k), str(n)]


@pytest.mark.parametrize("name", [x for x in MM if x.endswith(("-ALT", "-CoB"))])       # every such file: one that is not pinned fails
def test_alternative_basis_files_are_no_triples(name):
    rc, err = mmc(files(name))
    assert rc == NOT_TRIPLES[name], err
    if rc == 1:
        assert B.oracle_mod(B.load(name), B.P31)[0] > 0
    else:
        assert "outer dimension mismatch" in err


@pytest.mark.parametrize("name", [x for x in NAMES if re.match(r"\d+o\d+o\d+_", x)])      # every such file: one that is not pinned fails
def test_polynomial_triples_are_refused_or_fail(name):
    rc, err = mmc(files(name))
    assert rc == POLY[name], err
    assert ("outer dimension mismatch" in err) if rc == 3 else ("ERROR, not a" in err)


@pytest.mark.parametrize("name,which,i,j,value", [("2x2x2_7_Winograd", 0, 3, 1, 5), ("3x4x7_63_rational", 2, None, None, 0), ("4x4x4_49_156", 1, 48, 15, -2)])
def test_one_changed_entry(tmp_path, name, which, i, j, value):
    T0 = B.load(name)
    if value == 0:                                                             # the middle entry of the matrix goes
        keys = sorted(T0[which][2])
        i, j = keys[len(keys) // 2]
    T = B.changed(T0, which, i, j, value)
    q = 131071
    cnt, e, v = B.oracle_mod(T, q)
    assert cnt > 0
    f = B.write_triple(tmp_path, T)
    rc, err = mmc(["-q", q, "--count"] + f)
    m, k, n = T[3]
    assert rc == 1 and "ERROR, not a %dx%dx%d MM algorithm over Z/%dZ" % (m, k, n, q) in err
    ge, gidx, gsum, gexp = first_of(err)
    a, b, b2, c, a2, c2 = B.indices(e, T[3])
    assert (ge, gidx, gsum) == (e, (a, b, b2, c, a2, c2), str(v))
    assert gexp == int(a == a2 and b == b2 and c == c2)
    assert "# %d of %d equations violated" % (cnt, (m * k) * (k * n) * (m * n)) in err
    # over Q: the same equation (the change is far below the prime), its sum as a rational
    qc, qe, qv = B.oracle_q(T)
    rc, err = mmc(f)
    assert rc == 1 and first_of(err)[0] == qe and first_of(err)[2] == str(qv)
    # without --count the first equation is the same
    rc, err2 = mmc(["-q", q] + f)
    assert rc == 1 and first_of(err2)[:2] == (e, (a, b, b2, c, a2, c2)) and "equations violated" not in err2


@pytest.mark.parametrize("name", ["2x2x2_7_Winograd", "4x4x4_48_rational", "3x3x6_40"])
def test_certificate_line(name):
    T = B.load(name)
    beta, j = B.certificate(T)
    rc, err = mmc(files(name))
    assert rc == 0 and cert_of(err) == (beta, j, [B.P31][:j]), err


def test_certificate_of_rank_15096(tmp_path):
    """every +-1 triple needs one prime; for r = 15096, beta = 14 + 1 + 1 + 1 + 2 = 19 (here: 1x1x1 with 15095 empty products)"""
    one = {(0, 0): B.Fraction(1)}
    T = ((15096, 1, one), (15096, 1, one), (1, 15096, one), (1, 1, 1))
    assert B.certificate(T) == (19, 1)
    rc, err = mmc(B.write_triple(tmp_path, T))
    assert rc == 0 and cert_of(err) == (19, 1, [B.P31]) and "SUCCESS: correct 1x1x1 (3,0)" in err


def test_certificate_of_a_near_miss_takes_two_primes(tmp_path):
    """a +-1 triple with the first prime added to one entry: unchanged modulo that prime, wrong over Q"""
    T0 = B.load("2x2x2_7_Winograd")
    (t, x), v = sorted(T0[0][2].items())[0]
    T = B.changed(T0, 0, t, x, v + B.P31)
    beta, j = B.certificate(T)
    assert j == 2 and B.oracle_mod(T, B.P31)[0] == 0
    f = B.write_triple(tmp_path, T)
    rc, err = mmc(f)
    gb, gj, primes = cert_of(err)
    assert rc == 1 and (gb, gj) == (beta, 2), err
    assert primes[0] == B.P31 and primes[1] < B.P31 and all(pow(2, p - 1, p) == 1 for p in primes)
    assert not any(pow(2, p - 1, p) == 1 and pow(3, p - 1, p) == 1 for p in range(primes[1] + 1, B.P31))     # the largest prime below
    cnt, e, val = B.oracle_mod(T, primes[1])
    ge, _, gsum, _ = first_of(err)
    assert ge == e and "modulo %d: %d" % (primes[1], val) in err
    want = B.sum_at(T, e)                                                       # the rational at that equation, whichever is first over Q
    assert gsum == str(want) and B.residue(want, primes[1]) == val
    rc, err = mmc(["-q", B.P31] + f)                                           # the first prime alone passes
    assert rc == 0 and "SUCCESS" in err


def test_pair_ranges_compose(tmp_path):
    T = B.changed(B.changed(B.load("3x3x3_23_58"), 0, 2, 1, 7), 2, 8, 20, 3)
    q = B.P31
    f = B.write_triple(tmp_path, T)
    m, k, n = T[3]
    npairs = m * k * k * n
    full = B.oracle_mod(T, q)
    cut = full[1] // (m * n) + 1                                               # the first violated pair ends the first range
    assert 0 < cut < npairs
    got = []
    for p0, cnt in ((0, cut), (cut, npairs - cut)):
        rc, err = mmc(["-q", q, "--count", "--pairs", "%d:%d" % (p0, cnt)] + f)
        want = B.oracle_mod(T, q, p0, p0 + cnt)
        assert "[partial: pairs %d .. %d of %d]" % (p0, p0 + cnt - 1, npairs) in verdict(err)[0]
        assert rc == (1 if want[0] else 0)
        if want[0]:
            assert first_of(err)[0] == want[1] and "# %d of %d equations violated" % (want[0], cnt * m * n) in err
        got.append(want[0])
    assert sum(got) == full[0] and got[0] > 0
    rc, err = mmc(["-q", q, "--pairs", "%d:%d" % (cut, npairs)] + f)
    assert rc == 4 and "--pairs" in err
    T1 = B.load("3x3x3_23_58")                                                  # a correct triple: partial SUCCESS lines say so
    rc, err = mmc(["--pairs", "5:7"] + files("3x3x3_23_58"))
    assert rc == 0 and "SUCCESS: correct 3x3x3" in err and "[partial: pairs 5 .. 11 of 81]" in err and T1[3] == (3, 3, 3)


def test_dimension_mismatches(tmp_path):
    W = files("2x2x2_7_Winograd"); S = files("3x3x3_23_58")
    rc, err = mmc([W[0], S[1], W[2]])
    assert rc == 2 and "****** ERROR, inner dimension mismatch: 7(.)23|7 ******" in err
    T = B.load("2x2x2_7_Winograd")
    wide = (T[0][0], 6, T[0][2])                                               # L with 6 columns: n = floor(sqrt(4 4 / 6)) = 1
    f = B.write_triple(tmp_path, (wide, T[1], T[2], T[3]))
    rc, err = mmc(f)
    assert rc == 3 and "****** ERROR, outer dimension mismatch: 6:4x4 4:4x1 4:4x1 ******" in err


def test_refusals_and_help(tmp_path):
    W = files("2x2x2_7_Winograd")
    for opt in (["-P", "X^2-3"], ["-I", "Y"]):
        rc, err = mmc(opt + W)
        assert rc not in (0, 1, 2, 3) and "polynomial quotients (%s) are not supported" % opt[0] in err
    rc, err = mmc(["-b", 12] + W)                                              # accepted, no effect
    assert rc == 0 and "SUCCESS" in err
    rc, err = mmc(["-h"])
    assert "no randomness" in err
    third = B.write_triple(tmp_path, B.changed(B.load("2x2x2_7_Winograd"), 0, 0, 0, B.Fraction(1, 3)))   # a denominator that is no unit
    rc, err = mmc(["-q", 3] + third)
    assert rc == 4 and "not invertible modulo 3" in err
    rc, err = mmc(["-q", 16] + W)                                              # 16 -> 1 -> 2
    assert rc == 0 and "over Z/2Z" in err
    rc, err = mmc(["-q", 2 ** 40 + 15] + W)                                     # the 62-bit field of the host
    assert rc == 0 and "over Z/%dZ" % (2 ** 40 + 15) in err
    rc, err = mmc(["-r", 1, 10 ** 18, 0] + W, timeout=20)                        # 1^e - 0 = 1 -> 2, at once whatever e is
    assert rc == 0 and "over Z/2Z" in err
    rc, err = mmc(["-r", 0, 10 ** 18, 0] + W, timeout=20)
    assert rc == 4 and "modulus r^e - s is not positive" in err
    rc, err = mmc(["-r", 2, 10 ** 18, 1] + W, timeout=20)
    assert rc == 4 and "above 2^62" in err
    rc, err = mmc(["-q", 15] + W)                                              # a composite modulus
    assert rc == 0 and "over Z/15Z" in err
