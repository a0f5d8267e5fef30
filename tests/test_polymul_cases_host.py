"""The oracle of tests/polymul_lib.py on the polynomial-multiplication fixtures: the number of violated coefficient equations of
every line of the table below is pinned (0: the triple is correct), and the generators of that file give triples that the oracle
finds correct, padded or not, and wrong as soon as one entry changes.  No GPU, and nothing of the product."""
import random
from fractions import Fraction

import pytest

import polymul_lib as M


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_fixture_counts(case):
    name, q, f, count = case
    got = M.oracle(M.load(name), q, f)
    assert got[0] == count
    assert (got[1] is None) == (count == 0)


def test_the_first_equation_and_its_values():
    """the short product without X^3 misses its three top coefficients: (i, j, c) = (1, 2, 3), (2, 1, 3), (2, 2, 4)"""
    T = M.load("2o2o2_5_shortproduct")
    assert M.shape(T) == (3, 3, 3, 5)
    assert M.oracle(T) == (3, (1 * 3 + 2) * 5 + 3, 0, 1)
    assert M.oracle(T, pair0=6) == (2, (2 * 3 + 1) * 5 + 3, 0, 1)
    assert M.oracle(T, pair0=0, pair1=5) == (0, None, None, None)
    T = M.load("2o2o2_4_partSP")
    cnt, e, got, want = M.oracle(T, 0, M.X3)
    assert cnt == 2 and got != want and e < 27


def test_remainders_by_long_division():
    f = M.F243
    assert M.rem([0, 0, 0, 0, 0, 1], f, 0) == [-1, 1, 0, 0, 0]                   # X^5 = X - 1
    assert M.rem([0, 0, 0, 0, 0, 1], [c % 3 for c in map(int, f)], 3) == [2, 1, 0, 0, 0]
    assert M.rem([1, 2], f, 0) == [1, 2, 0, 0, 0]                                # shorter than f: padded
    assert M.rem([0] * 7 + [1], [Fraction(1, 2), 0, Fraction(-2, 3)], 0) == [0, Fraction(27, 64)]   # X^2 = 3/4, X^7 = (3/4)^3 X
    for e in range(12):
        assert M.power_mod(e, f) == M.rem([0] * e + [1], f, 0)
    assert M.poly_text(M.F243) == "1-X+X^5" and M.poly_text(M.F243M, "y") == "-1-y^2-y^3+y^4+y^5"
    assert M.poly_text(M.poly("1/2 0 -2/3")) == "1/2-2/3*X^2"


@pytest.mark.parametrize("na,nb", [(1, 1), (1, 4), (3, 2), (5, 5)])
def test_schoolbook(na, nb):
    T = M.schoolbook(na, nb)
    assert M.shape(T) == (na, nb, na + nb - 1, na + nb - 1)
    for q in (0, 2, 6, M.P31):
        assert M.oracle(T, q)[0] == 0
    if na * nb > 1:
        assert M.oracle(M.changed(T, 2, na + nb - 2, na * nb - 1, 2))[:2] == (1, na * nb * (na + nb - 1) - 1)   # the last equation
        assert M.oracle(M.with_rows(T, na + nb - 2))[0] == 1                                        # c = i + j >= nc
        assert M.oracle(M.with_rows(T, na + nb + 2))[0] == 0                                        # zero rows


@pytest.mark.parametrize("f", [M.F243, M.X3, M.poly("3 1"), M.poly("1/2 0 -2/3"), M.poly("1 0 0 0 0 0 0 0 0 0 0 7")], ids=M.poly_text)
def test_schoolbook_folded(f):
    T = M.schoolbook_folded(4, 3, f)
    d = len(f) - 1
    assert M.shape(T)[2] == d
    assert M.oracle(T, 0, f)[0] == 0
    assert M.oracle(T, M.P31, f)[0] == 0
    assert M.oracle(M.schoolbook(4, 3), 0, f)[0] == 0                              # and folding afterwards is right too
    (z, t), v = sorted(T[2][2].items())[-1]
    assert M.oracle(M.changed(T, 2, z, t, v + 1), 0, f)[0] >= 1


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_karatsuba(k):
    T = M.karatsuba(k)
    n = 2 ** k
    assert (T[0][0], T[0][1], T[2][0]) == (3 ** k, n, 2 * n - 1)
    assert M.oracle(T)[0] == 0 and M.oracle(T, 2)[0] == 0 and M.oracle(T, M.P31)[0] == 0
    if k:
        (t, x), v = sorted(T[0][2].items())[len(T[0][2]) // 2]
        assert M.oracle(M.changed(T, 0, t, x, v + 1))[0] > 0


def test_karatsuba_is_the_fixture():
    got, want = M.karatsuba(1), M.load("1o1o2_3_Karatsuba")
    assert M.shape(got) == M.shape(want) and got[0][0] == want[0][0] == 3


def test_paddings_keep_the_bilinear_map():
    rng = random.Random(5)
    T0 = M.karatsuba(2)
    T = M.scaled(T0, [Fraction(rng.randrange(1, 9), rng.randrange(1, 9)) * rng.choice((1, -1)) for _ in range(T0[0][0])])
    T = M.with_null_products(T, 70, 1, 2, rng)
    T = M.with_cancelling_pair(T, 7, 0, 3, rng)
    T = M.with_cancelling_pair(T, 1, 3, 3, rng)
    assert T[0][0] == 9 + 70 + 4
    assert len([1 for (t, x) in T[0][2] if x == 1]) >= 70 and len([1 for (z, t) in T[2][2] if t == 79]) == 7
    for q, f in ((0, None), (M.P31, None), (0, M.F243), (131071, M.X3)):
        assert M.oracle(T, q, f)[0] == 0
    assert M.oracle(M.changed(T, 2, 6, 80, 0))[0] > 0                              # a cancelling pair that no longer cancels
    D = M.with_full_cancelling_pairs(M.karatsuba(1), 3, rng)
    assert D[0][0] == 9 and len(D[0][2]) == 4 + 12 and len(D[2][2]) == 5 + 18 and M.oracle(D)[0] == 0 and M.oracle(D, 7, M.poly("1 1 1"))[0] == 0


@pytest.mark.parametrize("case", [c for c in M.CASES if c[1] == 0], ids=M.case_id)
def test_certificate_bounds_the_cleared_defect(case):
    """beta of DESIGN.md 2.13 against the largest coefficient it has to bound, computed over Q"""
    name, _, f, _ = case
    T = M.load(name)
    assert M.certificate(T, f)[0] >= M.cleared_defect_bits(T, f)
