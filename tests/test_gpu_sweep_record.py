"""The row record of plo::cse_big_kernel's sweeps (mode 2) and the aggregation probe, against the LITERAL oracle.

The row search writes one 16-byte record per rewritten row; its third word (PLO_RW_* in plo_cse_big.hip) carries what is constant
per row: the length, the +-1 flag and value index of the entry that the new column's entry inherits (the `l0` entry: the chosen
pair's column with MORE +-1 entries, the first one on a tie -- the +-1-count rule of include/plinopt_optimize.inl:70-88), and the
value indices `via`, `vib` of the two removed entries, from which the sweep forms its ratio-identifier index (rtid[via][vi] left of
the `a` entry, rtid[vi][via] right of it, chosen by POSITION).  One synthetic matrix reaches every field and every reader:

  values    exactly 32 distinct residues mod 131071 (mode 2's limit): +-{1,2,3,4,5,6,9,10,12,15,18,20,25,30,45,50}.  Value index =
            rank of the residue: index 0 is 1, index 31 is -1.  Ratios are asymmetric (2/3 != 3/2), so a transposed lookup
            changes a pair key, hence a frequency, hence the steps and the cost.
  groups    group g has f_g rows (identical pairs, so every triple has frequency >= 2) that hold columns a_g < b_g of its own with
            v_b = r_g v_a; f_g are distinct and above every other frequency, so the groups' prefix steps come first, in this order,
            while columns a_g and b_g are exactly as built -- the +-1 counts of the two columns are those of the group's rows:

              g  f   (v_a, v_b) per row pair, cycled                        +-1 in a / in b      value indices of (a, b)
              0  96  (2,1) (4,2) (6,3) (10,5) (30,15) (-2,-1)               fewer (0 < 32)       l0 = b
              1  80  (1,2) (2,4) (3,6) (5,10) (-1,-2) (15,30)               more                 l0 = a
              2  72  (1,-1)                                                  equal                (0, 31)
              3  64  (1,1)                                                   equal                (0, 0)
              4  56  (-1,-1)                                                 equal                (31, 31)
              5  48  (-1,1)                                                  equal                (31, 0)
              6  40  (3,15) (2,10) (1,5) (6,30) (-3,-15)                     more                 l0 = a
              7  24  (2,3) (4,6) (6,9) (10,15)    rows of exactly TWO entries: the new column's entry lands at position 0

            a_g = 30 + 50 g, b_g = a_g + 20 lie inside the range of the other columns, so a generic row has entries left of a,
            between a and b and right of b (the three position classes of a swept entry, in ONE row); every group of 0..6 also has
            rows where a is the first entry, rows where b is the last, and rows of two entries; group 0 has a pair of rows of 129
            entries and group 1 one of 65 (a row spans trips of 64 entries, a lane's row changes inside a trip).
  filler    120 pairs of 10 entries: triples enough for the plan to take the deferred updates (`merge_groups` > 0 says it did:
            the flat sweep ran).

Every run must give the oracle's (adds, muls) seed by seed.  PLO_BIG_AGGBITS=6 shrinks the LDS aggregation table to 64 slots: most
entries of the big steps then find no slot within their 8 pairs and go through direct retirement, which reads via and vib from the
record word as well (`spilled_pairs` > 0).  PLO_BIG_EAGER / NORID / IDKEYS / WIDE run the other sweeps and kernel instances over the
same records.
"""
import os
import random

import pytest

import synth
from plo_testlib import OracleMatrix

pytestmark = pytest.mark.gpu
P = 131071
NSEEDS = 8
SEED0 = 1
MAGS = (1, 2, 3, 4, 5, 6, 9, 10, 12, 15, 18, 20, 25, 30, 45, 50)
VALS = sorted({x % P for x in MAGS} | {P - x for x in MAGS})
NOTHER_MAX = 480                                            # columns 0..479: the groups' 16 and 464 others
GROUPS = (
    (96, ((2, 1), (4, 2), (6, 3), (10, 5), (30, 15), (-2, -1)), 129),
    (80, ((1, 2), (2, 4), (3, 6), (5, 10), (-1, -2), (15, 30)), 65),
    (72, ((1, -1),), 0),
    (64, ((1, 1),), 0),
    (56, ((-1, -1),), 0),
    (48, ((-1, 1),), 0),
    (40, ((3, 15), (2, 10), (1, 5), (6, 30), (-3, -15)), 0),
    (24, ((2, 3), (4, 6), (6, 9), (10, 15)), 0),
)
KNOBS = ("PLO_BIG_FWIN", "PLO_BIG_EAGER", "PLO_BIG_NORID", "PLO_BIG_IDKEYS", "PLO_BIG_VT_GLOBAL", "PLO_BIG_WIDE", "PLO_BIG_AGGBITS")


def _ab(g):
    return 30 + 50 * g, 50 + 50 * g


def _matrix():
    """rows as {column: value}, and per group the list of its row indices"""
    rng = random.Random(23)
    gcols = {c for g in range(len(GROUPS)) for c in _ab(g)}
    others = [c for c in range(NOTHER_MAX) if c not in gcols]
    rows, members = [], []
    for g, (f, pairs, long_len) in enumerate(GROUPS):
        a, b = _ab(g)
        lo, mid, hi = [c for c in others if c < a], [c for c in others if a < c < b], [c for c in others if c > b]
        mine = []
        for k in range(f // 2):
            va, vb = pairs[k % len(pairs)]
            if g == 7 or k % 8 == 3:
                cols = []                                   # exactly two entries
            elif k % 8 == 1:
                cols = rng.sample(mid + hi, 6)              # a is the first entry
            elif k % 8 == 2:
                cols = rng.sample(lo + mid, 6)              # b is the last entry
            else:
                n = long_len - 2 if (long_len and k == 0) else 6
                cols = [rng.choice(lo), rng.choice(mid), rng.choice(hi)]       # all three position classes in one row
                cols += rng.sample([c for c in others if c not in cols], n - 3)
            row = {c: rng.choice(VALS) for c in cols}
            row[a], row[b] = va % P, vb % P
            mine += [len(rows), len(rows) + 1]
            rows += [dict(row), dict(row)]
        members.append(mine)
    for _ in range(120):
        row = {c: rng.choice(VALS) for c in rng.sample(others, 10)}
        rows += [dict(row), dict(row)]
    return len(rows), NOTHER_MAX, rows, members


@pytest.fixture(scope="module")
def case():
    """the matrix in CSR and the oracle's costs of seeds 1..8, computed once"""
    m, n, rows, _ = _matrix()
    rp, c, v = synth.to_csr(rows, P)
    M = OracleMatrix(m, n, rp, c, v, P)
    want = tuple(M.cost_many(seed0=SEED0, nseeds=NSEEDS, nthreads=8))
    return (m, n, rp, c, v), want


def test_matrix_reaches_what_it_claims():
    """from the construction alone (no GPU): orientations, value indices, ratios, position classes, row lengths"""
    m, n, rows, members = _matrix()
    assert len(VALS) == 32 and {x for r in rows for x in r.values()} == set(VALS)          # exactly 32 distinct values: mode 2's limit
    assert VALS[0] == 1 and VALS[31] == P - 1
    inv = {x: pow(x, P - 2, P) for x in VALS}
    ratios = {x * inv[y] % P for x in VALS for y in VALS}
    assert len(ratios) < 1024
    assert any(x * inv[y] % P != y * inv[x] % P for x in VALS for y in VALS)               # asymmetric
    unit = (1, P - 1)
    orient, ends, shapes = set(), set(), set()
    for g, mine in enumerate(members):
        a, b = _ab(g)
        ua, ub = sum(rows[i][a] in unit for i in mine), sum(rows[i][b] in unit for i in mine)
        orient.add((ua > ub) - (ua < ub))
        ends |= {(VALS.index(rows[i][a]), VALS.index(rows[i][b])) for i in mine}
        for i in mine:
            cols = sorted(rows[i])
            shapes.add(("two", len(cols) == 2))
            shapes.add(("a first", cols[0] == a and len(cols) > 2))
            shapes.add(("b last", cols[-1] == b and len(cols) > 2))
            shapes.add(("three classes", cols[0] < a and any(a < c < b for c in cols) and cols[-1] > b))
            shapes.add(("len", len(cols)))
        # the group's prefix is the only triple of its frequency: nothing else holds its two columns
        assert all((a in r) == (b in r) == (i in mine) for i, r in enumerate(rows))
    assert orient == {-1, 0, 1}                                                            # swap true, swap false, the tie
    assert {(0, 0), (31, 31), (0, 31), (31, 0)} <= ends
    assert {("two", True), ("a first", True), ("b last", True), ("three classes", True), ("len", 65), ("len", 129)} <= shapes
    assert len({f for f, _, _ in GROUPS}) == len(GROUPS)


def _run(csr, env=None):
    from plinopt_amd import CSEPlan
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(env or {})
        m, n, rp, c, v = csr
        plan = CSEPlan(m, n, rp, c, v, P, hbm=True)           # PLO_PLAN_HBM
        assert plan.is_hbm
        got = plan.cost_many(seed0=SEED0, n=NSEEDS)
        cnt = plan.hbm_counters()
        plan.close()
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    print("HBM counters %s: %s" % (env or "default", cnt))
    return tuple(got), cnt


def _swept(cnt):
    """steps were made, the groups' prefix steps at least, and rows searched (a step rewrites >= 2 rows)"""
    return cnt["candidates"] >= 1 and cnt["steps"] >= cnt["candidates"] * len(GROUPS) and cnt["rows_searched"] >= 2 * cnt["steps"] and cnt["eager_refits"] == 0


def test_flat_sweep(hip, case):
    csr, want = case
    got, cnt = _run(csr)
    assert got == want
    assert _swept(cnt), cnt
    assert cnt["merge_groups"] > 0, cnt                      # deferred updates: the flat sweep is the one that ran
    assert cnt["spilled_pairs"] == 0, cnt                    # ... and its aggregation table took every entry


def test_direct_retirement(hip, case):
    """a 64-slot aggregation table: the entries that find no slot are retired directly, with via and vib from the record word"""
    csr, want = case
    got, cnt = _run(csr, {"PLO_BIG_AGGBITS": "6"})
    assert got == want
    assert _swept(cnt) and cnt["merge_groups"] > 0, cnt
    assert cnt["spilled_pairs"] > 0, cnt


@pytest.mark.parametrize("env", [{"PLO_BIG_EAGER": "1"}, {"PLO_BIG_NORID": "1"}, {"PLO_BIG_IDKEYS": "1"}, {"PLO_BIG_WIDE": "1"},
                                 {"PLO_BIG_IDKEYS": "1", "PLO_BIG_EAGER": "1"}],
                         ids=lambda e: "+".join(sorted(k[8:].lower() for k in e)))
def test_other_modes_and_instances(hip, case, env):
    """the two-rows sweep (eager table; no ratio identifiers: 32-byte records), identifier keys, 64-bit offsets: emit() is shared"""
    csr, want = case
    got, cnt = _run(csr, env)
    assert got == want
    assert _swept(cnt), cnt
    if "PLO_BIG_EAGER" in env:
        assert cnt["merge_groups"] == 0, cnt
    elif "PLO_BIG_NORID" not in env:
        assert cnt["merge_groups"] > 0, cnt
