"""The Brent equations on the GPU (plo_brent.hip, plo_brent_*, bin/MMchecker --gpu 1) against the independent oracle of
tests/brent_lib.py: (violated, first, value) must be the oracle's exactly, and the tool's text its own --gpu 0 text.  Every
positive input is shown correct by the oracle before the device is asked.  The shapes put the row length of P^T on both sides of
the wave width, mn on both sides of a chunk (PLO_BRENT_CHUNK, in child processes), q - 1 in every entry, violations at the
first and the last equation, and pair ranges that are no multiple of the waves of a workgroup."""
import json
import os
import re
import subprocess
import sys

import pytest

import brent_lib as B
from plo_testlib import DATA, ROOT

pytestmark = pytest.mark.gpu

MMC = os.path.join(ROOT, "bin", "MMchecker")
ANSI = re.compile(r"\x1b\[[0-9;]*m")
P31 = B.P31


def plan_of(T, q):
    from plinopt_amd import BrentPlan
    m, k, n = T[3]
    return BrentPlan(B.csr(T[0]), B.csr(T[1]), B.csr(T[2]), m, k, n, q)


def device(T, q, pair0=0, pair1=None):
    plan = plan_of(T, q)
    v, first, value, exp = plan.check(pair0, pair1)
    mn = T[3][0] * T[3][2]
    npairs = (plan.npairs if pair1 is None else pair1) - pair0
    assert plan.last_stats["candidates"] == npairs * mn
    if v:
        a, b, b2, c, a2, c2 = B.indices(first, T[3])
        assert exp == int(a == a2 and b == b2 and c == c2)
        return v, first, value
    return 0, None, None


def same(T, q, positive=None):
    want = B.oracle_mod(T, q)
    if positive is not None:
        assert (want[0] == 0) == positive
    assert device(T, q) == want
    return want


def tool(args, gpu, env=None):
    r = subprocess.run([MMC, "--gpu", str(gpu)] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)
    text = "".join(ln + "\n" for ln in ANSI.sub("", r.stderr).splitlines() if not ln.startswith(("# GPU:", "# host:")))
    return r.returncode, text, ANSI.sub("", r.stderr)


def tool_same(args):
    g, h = tool(args, 1), tool(args, 0)
    assert g[:2] == h[:2], (g, h)
    assert "# GPU: " in g[2] and "kernel " in g[2] and "# host: " in h[2]
    return g


def one_one_one():
    one = {(0, 0): B.Fraction(1)}
    return (1, 1, one), (1, 1, one), (1, 1, one), (1, 1, 1)


@pytest.mark.parametrize("name,q", [("1x1x1", P31), ("2x2x2_7_Winograd", P31), ("3x4x7_63_rational", 131071), ("3x4x7_63_rational", P31), ("4x4x4_49_156", P31),
                                    ("4x4x4_49_156", 6), ("2x2x2_7_DPS-accurate", 513083)])
def test_fixtures(hip, name, q):
    T = one_one_one() if name == "1x1x1" else B.load(name)
    same(T, q, positive=True)
    if name != "1x1x1":                                                        # and wrong ones: an entry changed in each matrix in turn
        for which in range(3):
            (i, j), v = sorted(T[which][2].items())[len(T[which][2]) // 3]
            same(B.changed(T, which, i, j, v + 1), q, positive=False)


def test_a_permuted_shape_is_refused(hip):
    """m != k != n: 3x4x7 taken as 7x4x3 does not fit the matrices"""
    T = B.load("3x4x7_63_rational")
    from plinopt_amd import capi
    with pytest.raises(capi.PloError) as e:
        plan_of((T[0], T[1], T[2], (7, 4, 3)), P31)
    assert e.value.code == capi.PLO_E_ARG


@pytest.mark.parametrize("mkn", [(1, 1, 63), (1, 1, 64), (1, 1, 65), (1, 1, 129), (2, 1, 33), (3, 2, 5)])
def test_dense_naive_triples(hip, mkn):
    """the naive algorithm after a random change of basis: every row of P^T has mn entries (63 .. 129)"""
    N = B.naive(*mkn)
    T = B.change_basis(N, P31, sum(mkn))
    mn = mkn[0] * mkn[2]
    assert len([1 for (z, t) in T[2][2] if t == 0]) == mn
    same(T, P31, positive=True)
    same(N, P31, positive=True)
    (i, j), v = sorted(T[1][2].items())[-1]
    same(B.changed(T, 1, i, j, v + 1), P31, positive=False)


@pytest.mark.parametrize("mkn", [(1, 1, 65), (3, 2, 5), (2, 3, 2)])
def test_entries_q_minus_one(hip, mkn):
    """L and P negated: every entry is q - 1 and every product goes through the 64-bit reduction"""
    L, R, P, sh = B.naive(*mkn)
    neg = lambda M: (M[0], M[1], {ij: B.Fraction(-1) for ij in M[2]})  # noqa: E731
    for q in (P31, 2147483647, 2147483646):                                     # the project's prime, 2^31 - 1, and an even modulus
        T = (neg(L), R, neg(P), sh)
        same(T, q, positive=True)
        big = (neg(L), (R[0], R[1], {ij: B.Fraction(q - 1) for ij in R[2]}), neg(P), sh)     # (q-1)^3 = -1: every diagonal equation gives q - 1
        want = same(big, q, positive=False)
        assert want[2] == q - 1


def test_placed_violations(hip):
    T = B.change_basis(B.naive(2, 3, 2), P31, 5)
    m, k, n = T[3]
    mk, kn, mn = m * k, k * n, m * n
    assert B.oracle_mod(T, P31)[0] == 0
    # only the first, only the last equation: one more product with a single entry in each matrix, on the sparse naive triple
    N = B.naive(2, 3, 2)
    r = N[0][0]
    first_only = (r + 1, mk, {**N[0][2], (r, 0): B.Fraction(1)}), (r + 1, kn, {**N[1][2], (r, 0): B.Fraction(1)}), (mn, r + 1, {**N[2][2], (0, r): B.Fraction(1)}), N[3]
    want = same(first_only, P31, positive=False)
    assert want == (1, 0, 2)
    last_only = (r + 1, mk, {**N[0][2], (r, mk - 1): B.Fraction(5)}), (r + 1, kn, {**N[1][2], (r, kn - 1): B.Fraction(1)}), (mn, r + 1, {**N[2][2], (mn - 1, r): B.Fraction(1)}), N[3]
    want = same(last_only, P31, positive=False)
    assert want == (1, mk * kn * mn - 1, 6)
    # an all-zero column of L: its diagonal equations give 0 instead of 1
    x0 = 3
    noc = (T[0][0], mk, {ij: v for ij, v in T[0][2].items() if ij[1] != x0}), T[1], T[2], T[3]
    want = same(noc, P31, positive=False)
    assert want[0] == n and want[2] == 0 and want[1] // (kn * mn) == x0
    # an empty row of P^T (a product that is never used)
    t0 = 4
    nop = T[0], T[1], (mn, T[2][1], {ij: v for ij, v in T[2][2].items() if ij[1] != t0}), T[3]
    same(nop, P31, positive=False)


def test_pair_ranges(hip):
    T0 = B.change_basis(B.naive(3, 2, 5), P31, 11)
    (i, j), v = sorted(T0[0][2].items())[7]
    T = B.changed(T0, 0, i, j, v + 3)
    m, k, n = T[3]
    npairs = m * k * k * n
    full = B.oracle_mod(T, P31)
    assert full[0] > 0
    plan = plan_of(T, P31)
    W = plan.info()["waves_per_wg"]
    assert W > 1 and plan.info()["mn"] == m * n and plan.info()["chunks"] == 1
    ranges = [(0, 1), (5, 6), (npairs - 1, npairs), (1, 1 + W + 1), (2, 2 + 2 * W + 3), (0, npairs)]
    cut = full[1] // (m * n) + 2
    ranges += [(0, cut), (cut, npairs)]
    got = {}
    for p0, p1 in ranges:
        want = B.oracle_mod(T, P31, p0, p1)
        v, first, value, _ = plan.check(p0, p1)
        got[(p0, p1)] = (v, first, value) if v else (0, None, None)
        assert got[(p0, p1)] == want, (p0, p1)
        assert plan.last_stats["candidates"] == (p1 - p0) * m * n
    a, b = got[(0, cut)], got[(cut, npairs)]
    assert a[0] + b[0] == full[0] and a[1:] == full[1:]


CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r]
import brent_lib as B
from plinopt_amd import BrentPlan, capi
capi.check(capi.lib().plo_init(0))
out = []
for mkn in ((1, 1, 65), (2, 1, 33)):
    T0 = B.change_basis(B.naive(*mkn), B.P31, 3)
    (i, j), v = sorted(T0[2][2].items())[-1]
    for T in (T0, B.changed(T0, 2, i, j, v + 1)):
        m, k, n = T[3]
        plan = BrentPlan(B.csr(T[0]), B.csr(T[1]), B.csr(T[2]), m, k, n, B.P31)
        v_, first, value, _ = plan.check()
        out.append({"mkn": mkn, "info": plan.info(), "got": [v_, first, value if v_ else None], "want": list(B.oracle_mod(T, B.P31)), "launches": plan.last_stats["launches"]})
print(json.dumps(out))
"""


@pytest.mark.parametrize("knobs,chunks", [({"PLO_BRENT_CHUNK": "33"}, 2), ({"PLO_BRENT_CHUNK": "22"}, 3), ({"PLO_BRENT_CHUNK": "64", "PLO_BRENT_PAIRS": "7"}, 2)])
def test_chunks_and_launches_in_a_child(knobs, chunks):
    """mn = 65 and 66 in 2 and 3 chunks per pair, and a range in several launches: the same results"""
    env = dict(os.environ, **knobs)
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = json.loads(r.stdout.splitlines()[-1])
    assert len(rows) == 4
    for row in rows:
        assert row["info"]["chunks"] == chunks and row["info"]["chunk"] == int(knobs["PLO_BRENT_CHUNK"])
        assert row["got"] == row["want"], row
        if "PLO_BRENT_PAIRS" in knobs:
            npairs = row["info"]["mk"] * row["info"]["kn"]
            assert row["info"]["pairs_per_launch"] == 7 and row["launches"] == -(-npairs // 7)
    assert rows[0]["want"][0] == 0 and rows[1]["want"][0] > 0


def test_tool_over_q(tmp_path):
    f = [os.path.join(DATA, "4x4x4_48_rational_%s.sms" % x) for x in "LRP"]
    T = B.load("4x4x4_48_rational")
    beta, j = B.certificate(T)
    rc, text, _ = tool_same(f)
    assert rc == 0 and "# certificate: beta = %d, j = %d, primes %d\n" % (beta, j, P31) in text and "SUCCESS: correct 4x4x4" in text
    # the near miss: unchanged modulo the first prime, wrong over Q
    W = B.load("2x2x2_7_Winograd")
    (t, x), v = sorted(W[0][2].items())[0]
    N = B.changed(W, 0, t, x, v + P31)
    assert B.certificate(N)[1] == 2 and B.oracle_mod(N, P31)[0] == 0 and B.oracle_q(N)[0] > 0
    g = B.write_triple(tmp_path, N)
    rc, text, _ = tool_same(g)
    assert rc == 1 and "j = 2, primes %d " % P31 in text and "ERROR, not a 2x2x2 MM algorithm over Q" in text
    rc, text, _ = tool_same(["-q", P31] + g)
    assert rc == 0 and "SUCCESS" in text


def test_tool_modular_counts_and_ranges(tmp_path):
    T0 = B.load("3x4x7_63_rational")
    (i, j), v = sorted(T0[1][2].items())[100]
    T = B.changed(T0, 1, i, j, v + 1)
    f = B.write_triple(tmp_path, T)
    cnt, e, val = B.oracle_mod(T, 131071)
    rc, text, _ = tool_same(["-q", 131071, "--count"] + f)
    assert rc == 1 and "# first violated equation e=%d:" % e in text and ", sum %d instead of" % val in text
    assert "# %d of %d equations violated" % (cnt, 12 * 28 * 21) in text
    rc, text, _ = tool_same(["-q", 131071, "--pairs", "0:%d" % (e // 21)] + f)           # the pairs before the first violated one
    assert rc == 0 and "[partial: pairs 0 .. %d of 336]" % (e // 21 - 1) in text
    rc, text, _ = tool_same(["-q", 131071, "--pairs", "%d:1" % (e // 21)] + f)
    assert rc == 1 and "# first violated equation e=%d:" % e in text
    rc, text, _ = tool(["-q", 2 ** 31 + 11] + [os.path.join(DATA, "3x4x7_63_rational_%s.sms" % x) for x in "LRP"], 1)   # announced, then the host loop
    assert rc == 0 and "# the device refuses this input (a modulus of 2^31 or more): host loop" in text and "SUCCESS: correct 3x4x7" in text


def test_orbiter_output_passes(tmp_path):
    """bin/orbiter -O 1000 on copies of a fixture, then bin/MMchecker on what it wrote"""
    import shutil
    src = [os.path.join(DATA, "3x3x3_23_58_%s.sms" % x) for x in "LRP"]
    dst = [str(tmp_path / os.path.basename(s)) for s in src]
    for s, d in zip(src, dst):
        shutil.copy(s, d)
    r = subprocess.run([os.path.join(ROOT, "bin", "orbiter"), "-O", "1000"] + dst, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = [d[:-4] + ".nnz.sms" for d in dst]
    assert "Rdcd. opt" in r.stderr and all(os.path.exists(o) for o in out), r.stderr   # among the 1000 candidates there is a sparser triple (171 entries against 175)
    rc, text, _ = tool_same(out)
    assert rc == 0 and "SUCCESS: correct 3x3x3" in text


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_tensor_6x6x12(hip, dense):
    """3x3x6_40 (x) Winograd: rank 280, 186,624 equations; densified, every row of P^T has 72 entries"""
    T = B.tensor_6x6x12_dense() if dense else B.tensor_6x6x12()
    assert T[3] == (6, 6, 12) and T[0][0] == 280
    same(T, P31, positive=True)
    (i, j), v = sorted(T[0][2].items())[len(T[0][2]) // 2]
    want = same(B.changed(T, 0, i, j, v + 1), P31, positive=False)
    assert want[0] > 0
