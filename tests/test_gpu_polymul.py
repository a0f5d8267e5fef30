"""The coefficient equations of polynomial multiplication on the GPU (plo_polymul.hip, plo_polymul_*, bin/PMchecker --gpu 1)
against the independent oracle of tests/polymul_lib.py: (violated, first, value, expected) must be the oracle's exactly, and
the tool's text its own --gpu 0 text.  Every positive input is shown correct by the oracle before the device is asked.  The
shapes put the columns of L and R and the rows of P^T on both sides of the wave width, nc on both sides of a chunk
(PLO_POLYMUL_CHUNK, in child processes), the degree of f on both sides of the wave width and of Z, q - 1 in every entry,
violations at the first and the last equation, and pair ranges that are no multiple of the waves of a workgroup."""
import json
import os
import random
import re
import subprocess
import sys
from fractions import Fraction

import pytest

import polymul_lib as M
from plo_testlib import ROOT

pytestmark = pytest.mark.gpu

PMC = os.path.join(ROOT, "bin", "PMchecker")
ANSI = re.compile(r"\x1b\[[0-9;]*m")
P31 = M.P31


def plan_of(T, q, f=None):
    from plinopt_amd import PolyMulPlan
    return PolyMulPlan(M.csr(T[0]), M.csr(T[1]), M.csr(T[2]), q, M.plan_poly(f))


def device(T, q, f=None, pair0=0, pair1=None, plan=None):
    plan = plan or plan_of(T, q, f)
    v, first, value, exp = plan.check(pair0, pair1)
    w = M.width(T, f)
    info = plan.info()
    assert info["w"] == w and info["npairs"] == T[0][1] * T[1][1] and info["fold"] == int(bool(f) and len(f) - 1 < M.shape(T)[3])
    npairs = (plan.npairs if pair1 is None else pair1) - pair0
    assert plan.last_stats["candidates"] == npairs * w
    return (v, first, value, exp) if v else (0, None, None, None)


def same(T, q, f=None, positive=None):
    want = M.oracle(T, q, f)
    if positive is not None:
        assert (want[0] == 0) == positive
    assert device(T, q, f) == want
    return want


def small_poly(d, rng, lead=1):
    """a polynomial of degree d with coefficients in -3 .. 3, a constant term that is not 0, and the given leading coefficient"""
    return [Fraction(rng.choice((-3, -2, -1, 1, 2, 3)))] + [Fraction(rng.randrange(-3, 4)) for _ in range(d - 1)] + [Fraction(lead)]


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_fixtures(hip, case):
    """every line of the table; what is checked over Q is checked here modulo the first certificate prime"""
    name, q, f, count = case
    T = M.load(name)
    q = q or P31
    want = same(T, q, f, positive=(count == 0))
    assert want[0] == count                                                    # (the changes of the negatives are far below the prime)
    if count == 0:                                                             # and wrong ones: an entry changed in each matrix in turn
        bad = 0
        for which in range(3):
            (i, j), v = sorted(T[which][2].items())[len(T[which][2]) // 3]
            bad += same(M.changed(T, which, i, j, v + 1), q, f)[0] > 0
        assert bad > 0


def test_one_o_one_o_one(hip):
    one = {(0, 0): Fraction(1)}
    T = ((1, 1, dict(one)), (1, 1, dict(one)), (1, 1, dict(one)))
    assert same(T, P31, positive=True) == (0, None, None, None)
    assert same(T, 2, M.poly("-3 1"), positive=True)[0] == 0                   # d = Z = 1: nothing folds
    assert same(M.changed(T, 2, 0, 0, 5), P31, positive=False) == (1, 0, 5, 1)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_long_columns_that_share_their_products(hip, n):
    """column 1 of L and column 1 of R with n entries each, all on the same t (Karatsuba's two and n - 2 null products)"""
    rng = random.Random(n)
    T = M.with_null_products(M.karatsuba(1), n - 2, 1, 1, rng, 1, P31)
    assert len([1 for (t, x) in T[0][2] if x == 1]) == n and len([1 for (t, y) in T[1][2] if y == 1]) == n
    f = M.poly("1 0 1")
    same(T, P31, positive=True)
    same(T, P31, f, positive=True)
    r = T[0][0]
    B = M.changed(T, 2, 2, r - 1, 3)                                           # the last null product is none any more
    want = same(B, P31, positive=False)
    assert want[0] == 1 and want[1] == 3 * 3 + 2
    same(B, P31, f, positive=False)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_long_rows_of_pt(hip, n):
    """two cancelling products whose columns of P have n entries; P has 70 rows, those from 3 on must stay zero"""
    rng = random.Random(n)
    T = M.with_cancelling_pair(M.with_rows(M.schoolbook(2, 2), 70), n, 1, 0, rng, 1, P31)
    r = T[0][0]
    assert len([1 for (z, t) in T[2][2] if t == r - 1]) == n
    f = small_poly(4, rng)
    same(T, P31, positive=True)
    same(T, P31, f, positive=True)
    (z, t), v = max((k, v) for k, v in T[2][2].items() if k[1] == r - 1)       # the last entry of the row: the pair no longer cancels there
    want = same(M.changed(T, 2, z, t, v + 1), P31, positive=False)
    assert want[0] == 1 and want[1] == (1 * 2 + 0) * 70 + z
    same(M.changed(T, 2, z, t, v + 1), P31, f, positive=False)


@pytest.mark.parametrize("d", [1, 2, 63, 64, 65])
def test_degrees_around_the_wave_width(hip, d):
    """40 x 30 coefficients (Z = 69), every product scaled, folded modulo f of degree d: the lanes over c"""
    rng = random.Random(d)
    T0 = M.schoolbook(40, 30)
    T = M.scaled(T0, [Fraction(rng.randrange(1, 50) * rng.choice((1, -1))) for _ in range(T0[0][0])])
    f = small_poly(d, rng, lead=2)
    want = same(T, P31, f, positive=True)
    assert want[0] == 0
    (z, t), v = sorted(T[2][2].items())[-1]                                    # X^68, in the pair (39, 29) alone
    want = same(M.changed(T, 2, z, t, v * 2), P31, f, positive=False)
    assert want[1] // d == 40 * 30 - 1


def test_degrees_around_z(hip):
    """nested Karatsuba of depth 2 (Z = 7): d = Z - 1 folds one row; d = Z and d = Z + 3 fold nothing and have the width d"""
    rng = random.Random(3)
    T = M.karatsuba(2)
    (t, x), v = sorted(T[1][2].items())[4]
    B = M.changed(T, 1, t, x, v + 2)
    for d, fold in ((6, 1), (7, 0), (10, 0)):
        f = small_poly(d, rng, lead=3)
        plan = plan_of(T, P31, f)
        assert plan.info()["fold"] == fold and plan.info()["w"] == d
        same(T, P31, f, positive=True)
        want = same(B, P31, f, positive=False)
        assert want[0] > 0


def test_rows_of_p_beside_the_product_length(hip):
    rng = random.Random(8)
    S = M.scaled(M.schoolbook(3, 3), [Fraction(rng.randrange(2, 9)) for _ in range(9)])
    f = small_poly(4, rng)
    # nc > na + nb - 1: rows that must be zero, and one that is not
    more = M.with_rows(S, 9)
    assert same(more, P31, positive=True)[0] == 0 and same(more, P31, f, positive=True)[0] == 0
    one = M.changed(more, 2, 8, 4, 1)
    assert same(one, P31, positive=False)[:2] == (1, (1 * 3 + 1) * 9 + 8)
    assert same(one, P31, f, positive=False)[0] >= 1
    # nc < na + nb - 1 without f: violations at c = i + j >= nc, one per pair with i + j >= 3
    less = M.with_rows(S, 3)
    assert same(less, P31, positive=False) == (3, (1 * 3 + 2) * 5 + 3, 0, 1)
    # nc < d: with a fold (d < Z) such a P has lost coefficients; without one (d >= Z) the width d goes beyond nc
    assert same(less, P31, f, positive=False)[0] > 0
    assert same(M.schoolbook_folded(3, 3, f), P31, f, positive=True)[0] == 0   # nc = d: P folded beforehand
    assert same(S, P31, small_poly(8, rng), positive=True)[0] == 0             # nc = 5 < d = 8


def test_small_and_composite_moduli(hip):
    T = M.karatsuba(3)
    same(T, 2, positive=True)
    same(T, 2, M.F32S, positive=True)
    (t, x), v = sorted(T[0][2].items())[10]
    assert same(M.changed(T, 0, t, x, 0), 2, M.F32S, positive=False)[0] > 0
    f6 = M.poly("2 3 0 5")                                                     # q = 6: the leading coefficient 5 is a unit, 2 and 3 are zero divisors
    same(T, 6, positive=True)
    same(T, 6, f6, positive=True)
    assert same(M.changed(T, 0, t, x, 3), 6, f6)[0] == M.oracle(M.changed(T, 0, t, x, 3), 6, f6)[0]
    assert same(M.all_entries(M.schoolbook(3, 3), 3), 6, f6, positive=False)[0] > 0   # 3 . 3 . 3 = 3: sums of zero divisors


@pytest.mark.parametrize("q", [2147483647, P31, 2147483646])
def test_entries_q_minus_one(hip, q):
    """L and P negated: every entry is q - 1 and every product goes through the 64-bit reduction; so do the folds by f = -X^3 - X - 1"""
    L, R, P = M.schoolbook(5, 4)
    neg = lambda A: (A[0], A[1], {ij: Fraction(-1) for ij in A[2]})  # noqa: E731
    f = M.poly("-1 -1 0 -1")
    T = (neg(L), R, neg(P))
    same(T, q, positive=True)
    same(T, q, f, positive=True)
    big = M.all_entries((L, R, P), q - 1)                                      # (q - 1)^3 = -1: every pair finds q - 1 at c = i + j
    want = same(big, q, positive=False)
    assert want[2:] == (q - 1, 1) and want[0] == 20
    want = same(big, q, f, positive=False)
    assert want[2:] == (q - 1, 1)


def test_placed_violations(hip):
    S = M.schoolbook(3, 3)
    r, f = 9, M.poly("0 -1 0 1")                                               # X^3 = X, X^4 = X^2
    first = M.grown(S, 1)
    first[0][2][(r, 0)] = first[1][2][(r, 0)] = first[2][2][(0, r)] = Fraction(1)
    assert same(first, P31, positive=False) == (1, 0, 2, 1)
    assert same(first, P31, f, positive=False) == (1, 0, 2, 1)
    last = M.grown(S, 1)
    last[0][2][(r, 2)] = Fraction(5); last[1][2][(r, 2)] = last[2][2][(4, r)] = Fraction(1)
    assert same(last, P31, positive=False) == (1, 9 * 5 - 1, 6, 1)
    assert same(last, P31, f, positive=False) == (1, 9 * 3 - 1, 6, 1)
    # an all-zero column of L: its pairs find 0 where 1 is expected
    noc = ((9, 3, {ij: v for ij, v in S[0][2].items() if ij[1] != 1}), S[1], S[2])
    want = same(noc, P31, positive=False)
    assert want == (3, (1 * 3 + 0) * 5 + 1, 0, 1)
    # an empty row of P^T (a product that is never used)
    nop = (S[0], S[1], (5, 9, {ij: v for ij, v in S[2][2].items() if ij[1] != 4}))
    assert same(nop, P31, f, positive=False)[0] == 1


@pytest.mark.parametrize("f", [None, M.F243], ids=["plain", "folded"])
def test_pair_ranges(hip, f):
    T0 = M.karatsuba(3)
    (t, x), v = sorted(T0[0][2].items())[20]
    T = M.changed(T0, 0, t, x, v + 3)
    npairs, w = 64, M.width(T, f)
    full = M.oracle(T, P31, f)
    assert full[0] > 0
    plan = plan_of(T, P31, f)
    W = plan.info()["waves_per_wg"]
    assert W > 1 and plan.info()["chunks"] == 1
    cut = min(full[1] // w + 2, npairs - 1)
    ranges = [(0, 1), (5, 6), (npairs - 1, npairs), (1, 1 + W + 1), (2, 2 + 2 * W + 3), (0, npairs), (0, cut), (cut, npairs)]
    got = {}
    for p0, p1 in ranges:
        got[(p0, p1)] = device(T, P31, f, p0, p1, plan=plan)
        assert got[(p0, p1)] == M.oracle(T, P31, f, p0, p1), (p0, p1)
    a, b = got[(0, cut)], got[(cut, npairs)]
    assert a[0] + b[0] == full[0] and a[1:] == full[1:]


@pytest.mark.parametrize("f", [None, M.F243, M.poly("1 1 0 0 0 0 0 0 0 0 0 0 0 0 1")], ids=["plain", "d5", "d14"])
def test_nested_karatsuba_27x8(hip, f):
    rng = random.Random(27)
    T0 = M.karatsuba(3)
    assert (T0[0][0], T0[0][1], T0[2][0]) == (27, 8, 15)
    T = M.scaled(T0, [Fraction(rng.randrange(1, 1000), rng.randrange(1, 1000)) for _ in range(27)])
    same(T, P31, f, positive=True)
    same(T, 131071, f, positive=True)
    (z, t), v = sorted(T[2][2].items())[len(T[2][2]) // 2]
    assert same(M.changed(T, 2, z, t, v + 1), P31, f, positive=False)[0] > 0


CHILD = r"""
import json, random, sys
from fractions import Fraction
sys.path[:0] = [%r, %r]
import polymul_lib as M
from plinopt_amd import PolyMulPlan, capi
capi.check(capi.lib().plo_init(0))
rng = random.Random(1)
out = []
S = M.scaled(M.schoolbook(5, 5), [Fraction(rng.randrange(2, 99)) for _ in range(25)])          # na + nb - 1 = 9
for nc in (7, 8, 9, 17):
    T0 = M.with_rows(S, nc)
    (z, t), v = sorted(T0[2][2].items())[-1]
    for T in (T0, M.changed(T0, 2, z, t, v + 1)):
        for f in (None, M.poly("2 -1 0 1"), M.poly("1 0 3 0 0 0 0 0 0 0 1"), M.poly("1 " + "0 " * 19 + "1")):   # no fold; d = 3; d = 10 (beyond a chunk); d = 20 >= Z
            plan = PolyMulPlan(M.csr(T[0]), M.csr(T[1]), M.csr(T[2]), M.P31, M.plan_poly(f))
            v_, first, value, exp = plan.check()
            out.append({"nc": nc, "d": len(f) - 1 if f else 0, "info": plan.info(), "got": [v_, first, value if v_ else None, exp if v_ else None],
                        "want": list(M.oracle(T, M.P31, f)), "launches": plan.last_stats["launches"]})
print(json.dumps(out))
"""


@pytest.mark.parametrize("knobs", [{"PLO_POLYMUL_CHUNK": "8"}, {"PLO_POLYMUL_CHUNK": "8", "PLO_POLYMUL_PAIRS": "7"}, {"PLO_POLYMUL_CHUNK": "3"}], ids=["chunk8", "chunk8-pairs7", "chunk3"])
def test_chunks_and_launches_in_a_child(knobs):
    """nc = 7, 8, 9 and 17 with 8 (and 3) sums per chunk, plain and folded modulo f of degree 3 and 10 (F lives across the chunks)
    and unfolded over the width 20; and a range in several launches: the same results"""
    env = dict(os.environ, **knobs)
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = json.loads(r.stdout.splitlines()[-1])
    assert len(rows) == 32
    chunk = int(knobs["PLO_POLYMUL_CHUNK"])
    for row in rows:
        nc, d, info = row["nc"], row["d"], row["info"]
        Z = max(nc, 9)
        fold = 0 < d < Z
        walked = nc if fold else (d or Z)
        assert info["fold"] == int(fold) and info["w"] == (d or Z)
        assert info["chunk"] == min(chunk, walked) and info["chunks"] == -(-walked // info["chunk"])
        assert row["got"] == row["want"], row
        if "PLO_POLYMUL_PAIRS" in knobs:
            assert info["pairs_per_launch"] == 7 and row["launches"] == -(-25 // 7)
    assert any(row["info"]["chunks"] >= 3 and row["info"]["fold"] for row in rows)
    assert [row["want"][0] == 0 for row in rows if row["nc"] >= 9][:4] == [True] * 4       # nc = 9, unchanged: correct whatever f


def tool(args, gpu, env=None):
    r = subprocess.run([PMC, "--gpu", str(gpu)] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)
    text = "".join(ln + "\n" for ln in ANSI.sub("", r.stderr).splitlines() if not ln.startswith(("# GPU:", "# host:")))
    return r.returncode, text, ANSI.sub("", r.stderr)


def tool_same(args):
    g, h = tool(args, 1), tool(args, 0)
    assert g[:2] == h[:2], (g, h)
    assert "# GPU: " in g[2] and "kernel " in g[2] and "# host: " in h[2]
    return g


def test_the_four_pmcheck_lines_on_the_gpu():
    for name, opts in (("4o4o8_Toom5", []), ("4o4o8_Montgomery-13", []), ("4o4o4_F243-11-44", ["-q", "3", "-P", "1-X+X^5"]),
                       ("4o4o4_F243-Montgomery-13-42", ["-q", "3", "-P", "X^5+X^4-X^3-X^2-1"])):
        r = subprocess.run([PMC] + M.files(name) + opts, capture_output=True, text=True, timeout=120)   # as the reference writes them: --gpu 1 is the default
        err = ANSI.sub("", r.stderr)
        assert r.returncode == 0 and "# SUCCESS: correct %s Polynomial-Multiplication over" % name[:5] in err and "# GPU: " in err, err


TOOL_CASES = {("4o4o8_Toom5", 0, False), ("4o4o8_Toom5", 0, True), ("4o4o4_F243-11-44", 3, True), ("4o4o8_Montgomery-13", 7, False),
              ("2o2o2_5_shortproduct", 0, False), ("4o4o4_F243-Montgomery-13-42", 0, True), ("4o4o4_S243_10-43", 3, True), ("3o3o3_S81_8_22", 3, True)}


@pytest.mark.parametrize("case", [c for c in M.CASES if (c[0], c[1], bool(c[2])) in TOOL_CASES], ids=M.case_id)
def test_tool_text_is_the_hosts(case):
    """positives and negatives, over Q and modulo q, with and without a polynomial"""
    name, q, f, count = case
    args = (["-q", q] if q else []) + (["-P", M.poly_text(f)] if f else []) + ["--count"] + M.files(name)
    rc, text, _ = tool_same(args)
    assert rc == (1 if count else 0)
    assert ("SUCCESS" in text) == (count == 0)
    if count:
        assert "# %d of " % count in text


def test_tool_near_miss_and_ranges(tmp_path):
    """the certificate's second prime at work on the device, and --pairs"""
    T0 = M.load("4o4o8_Toom5")
    (z, t), v = [x for x in sorted(T0[2][2].items()) if x[1].denominator == 1][1]
    g = M.write_triple(tmp_path, M.changed(T0, 2, z, t, v + P31))
    for opts in ([], ["-P", "1-X+X^5"]):
        rc, text, _ = tool_same(opts + g)
        assert rc == 1 and "# pass 1 of" in text and "modulo %d: no violated equation" % P31 in text and "# pass 2 of" in text and "ERROR, not a 4o4o8 MM algorithm over Q" in text
    rc, text, _ = tool_same(["-q", 3, "-P", "1-X+X^5", "--pairs", "3:6", "--count"] + M.files("4o4o4_S243_10-43"))
    want = M.oracle(M.load("4o4o4_S243_10-43"), 3, M.F243, 3, 9)
    assert "[partial: pairs 3 .. 8 of 25]" in text and rc == (1 if want[0] else 0)
    rc, text, _ = tool(["-q", 2 ** 31 + 11] + M.files("4o4o8_Montgomery-13"), 1)      # announced, then the host loop
    assert rc == 0 and "# the device refuses this input (a modulus of 2^31 or more): host loop" in text and "SUCCESS: correct 4o4o8" in text
