"""The wave prefix sums of plo::cse_big_kernel (wave_incl_scan: six v_add_u32_dpp, rows of 16 lanes joined by row_bcast:15 and
row_bcast:31) and the row-end store of the flat sweep, against the LITERAL oracle (OracleMatrix.cost_many), on the HBM family
(PLO_PLAN_HBM).

1. Tie pick, `cntM` scan (lane = first column mod 64): identical row pairs over 200 columns whose top level is two triples of
   frequency 8, (a, b) and (a, c), for each of the first columns a = 15, 16, 31, 32, 47, 48 (both sides of the three edges
   between the DPP rows of a wave), 63, 64 and 130 (column blocks 1 and 2).  The two triples of a group share half of their
   rows, so the one taken first halves the other: the picks show in the costs (16 different cost pairs among the 64 seeds).
   The first draw of every seed is computed here from the stream of DESIGN.md (Randomness) BEFORE the GPU runs, and the 64
   seeds must pick every one of the nine first columns first: a condition of the test, not a measurement.
2. Tie pick, block sums (512 sums of 64 columns, 8 per lane: lane = first column / 512): 48 rows over 24,600 columns, built
   the same way with frequency 4; the tied first columns 100, 8191, 8192, 16383, 16384, 24575, 24576 lie in lanes 0, 15 | 16,
   31 | 32, 47 | 48; same cover condition.
3. Row-end store (the new column's entry, written once per row at the end of a wave's batch of 64 rows): the first step
   rewrites 600 rows of 2 to 9 entries -- 75 rows per wave, a second batch of 11.  Rows are kept in column order and a < b, so
   the a entry is last in no row; what varies is the word at position L - 2 that the store overwrites: the a entry (a and b
   are the row's last two entries, rows of two entries among them: the new entry lands at position 0), the b entry (one entry
   behind b) or neither, and whether the b entry is the row's last.  All of these must occur (checked on the matrix).  With
   PLO_BIG_FWIN=128 a batch of some 350 entries is three windows, so that most row ends fall in windows before the batch's
   last; PLO_BIG_WIDE and PLO_BIG_IDKEYS take the other kernel instances.
4. Merge scans on the same matrix (large enough for the deferred plan: `merge_groups` > 0): PLO_BIG_LGRP=64 makes a group of
   every partition, i.e. as many calls of bounds() as a merge can have; PLO_BIG_LOGTRIG=2000 forces a merge whenever the log
   holds 2000 records, i.e. many short rounds of the partition pass.
"""
import os
import random

import pytest

import synth
from plo_testlib import OracleMatrix

pytestmark = pytest.mark.gpu
P = 131071
KNOBS = ("PLO_BIG_FWIN", "PLO_BIG_WIDE", "PLO_BIG_IDKEYS", "PLO_BIG_LGRP", "PLO_BIG_LOGTRIG", "PLO_BIG_EAGER", "PLO_BIG_NORID", "PLO_BIG_VT_GLOBAL")
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ the stream of DESIGN.md
def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def first_draw(seed):
    """next() of a fresh stream: state0 = 1 + splitmix64(seed) mod (2^31 - 2), next = 950706376 state mod (2^31 - 1)"""
    state0 = 1 + _splitmix64(seed) % 2147483646
    return 950706376 * state0 % 2147483647


def top_level(rows):
    """(M, the triples of frequency M in std::map order) of rows given as {column: value}; a triple is (col_a, col_b, ratio).  The
    ratio is only compared for equality here (v_a / v_b): the tests use top levels whose column pairs are all different, so that
    the order of the ties is the order of (col_a, col_b) whatever the ratio's definition."""
    cnt = {}
    for r in rows:
        it = sorted(r.items())
        for i in range(len(it)):
            for j in range(i + 1, len(it)):
                k = (it[i][0], it[j][0], it[i][1] * pow(it[j][1], -1, P) % P)
                cnt[k] = cnt.get(k, 0) + 1
    M = max(cnt.values())
    ties = sorted(k for k, c in cnt.items() if c == M)
    assert len({k[:2] for k in ties}) == len(ties)
    return M, ties


def first_picks(rows, seeds):
    """the first column of the triple that each seed's first step takes"""
    M, ties = top_level(rows)
    return M, ties, [ties[first_draw(s) % len(ties)][0] for s in seeds]


def _tied_matrix(rng, firsts, second, third, q, pool, extras, fillers):
    """For every a of `firsts`, with b = second(a) and c = third(a): q identical pairs of rows hold {a, b}, q pairs {a, b, c} and
    q pairs {a, c}, all with value 1, so that (a, b) and (a, c) both have frequency 4 q and share half of their rows: the one taken
    first halves the other, and which of the two that is -- the tie pick's choice -- decides how the group's rows go on.  Every
    pair of rows has extras[0] to extras[1] further entries from the few columns of `pool`, shared by all groups (no column twice
    in one group: a triple of a and a pool column has frequency 2), so that the two ways cost differently (the tests assert that
    the seeds' costs differ: a wrong pick would show).  `fillers` more pairs of three entries from the pool."""
    cols = [x for a in firsts for x in (a, second(a), third(a))]
    assert len(set(cols)) == len(cols) and not set(pool) & set(cols)
    rows = []
    for a in firsts:
        deal = rng.sample(pool, len(pool))
        for part in ((a, second(a)), (a, second(a), third(a)), (a, third(a))):
            for _ in range(q):
                row = {x: 1 for x in part}
                for _ in range(rng.randint(*extras)):
                    row[deal.pop()] = rng.choice([1, P - 1, 2])
                rows += [dict(row), dict(row)]
    for _ in range(fillers):
        row = {x: rng.choice([1, P - 1, 2]) for x in rng.sample(pool, 3)}
        rows += [dict(row), dict(row)]
    rng.shuffle(rows)
    return rows


def _run(csr, seed0, n, env=None):
    from plinopt_amd import CSEPlan
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(env or {})
        m, nn, rp, c, v = csr
        plan = CSEPlan(m, nn, rp, c, v, P, hbm=True)          # PLO_PLAN_HBM
        assert plan.is_hbm
        got = plan.cost_many(seed0=seed0, n=n)
        cnt = plan.hbm_counters()
        plan.close()
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    print("HBM counters %s: %s" % (env or "default", cnt))
    return tuple(got), cnt


def _tie_case(rows, ncols, seed0, nseeds):
    rp, c, v = synth.to_csr(rows, P)
    M = OracleMatrix(len(rows), ncols, rp, c, v, P)
    want = tuple(M.cost_many(seed0=seed0, nseeds=nseeds, nthreads=8))
    return (len(rows), ncols, rp, c, v), want


# ------------------------------------------------------------------------------------------------ 1. cntM across the DPP rows
CNTM_FIRSTS = (15, 16, 31, 32, 47, 48, 63, 64, 130)
CBLK_FIRSTS = (100, 8191, 8192, 16383, 16384, 24575, 24576)
TIE_SEED0, TIE_NSEEDS = 1, 64


def _tie_pick_test(rows, ncols, firsts, M0):
    seeds = range(TIE_SEED0, TIE_SEED0 + TIE_NSEEDS)
    M, ties, picks = first_picks(rows, seeds)
    assert M == M0 and tuple(k[0] for k in ties) == tuple(a for a in firsts for _ in range(2)), (M, ties)     # (a, b) and (a, c) of every group
    print("first picks of seeds %d..%d: %s" % (seeds[0], seeds[-1], picks))
    for a in firsts:
        assert a in picks, (a, picks)                         # both sides of every edge, the first lane and the last column
    csr, want = _tie_case(rows, ncols, TIE_SEED0, TIE_NSEEDS)
    print("oracle costs:", sorted(set(zip(*want))))
    assert len(set(zip(*want))) >= 4                         # the picks show in the costs
    got, cnt = _run(csr, TIE_SEED0, TIE_NSEEDS)
    assert got == want
    assert cnt["candidates"] == TIE_NSEEDS and cnt["steps"] >= TIE_NSEEDS * len(firsts), cnt


def test_cntm_scan_across_dpp_row_edges(hip):
    i = CNTM_FIRSTS.index
    rows = _tied_matrix(random.Random(5), CNTM_FIRSTS, lambda a: 140 + i(a), lambda a: 150 + i(a), 2, list(range(170, 200)), (1, 3), 10)
    _tie_pick_test(rows, 200, CNTM_FIRSTS, 8)


# ------------------------------------------------------------------------------------------------ 2. the block sums, lane = column / 512
def test_block_sum_scan_across_dpp_row_edges(hip):
    assert [a // 512 for a in CBLK_FIRSTS] == [0, 15, 16, 31, 32, 47, 48]
    rows = _tied_matrix(random.Random(6), CBLK_FIRSTS, lambda a: a + 7, lambda a: a + 14, 1, list(range(300, 306)) + list(range(12000, 12006)), (1, 2), 3)
    assert 24 <= len(rows) <= 48
    _tie_pick_test(rows, 24600, CBLK_FIRSTS, 4)


# ------------------------------------------------------------------------------------------------ 3. and 4. the 600-row step
BIG_SEED0, BIG_NSEEDS = 1, 8
BIG_A, BIG_B, BIG_NCOLS = 150, 250, 420


def _big_matrix():
    """300 identical pairs of rows of 2..9 entries that hold columns 150 and 250 with one ratio (the first step takes that pair and
    rewrites the 600 rows), their other entries before a, between a and b or behind b; 420 filler pairs of 10 entries give the
    plan the distinct triples it wants for the deferred updates"""
    rng = random.Random(23)
    vals = [1, P - 1, 2, P - 2, 3]
    pick = [1, P - 1] * 4 + vals
    other = [c for c in range(BIG_NCOLS) if c not in (BIG_A, BIG_B)]
    rows, ends = [], set()
    for i in range(300):
        L = 2 + i % 8
        tail = i % 3                                          # entries behind b: none (b is last), one (b sits at L - 2), two
        behind = rng.sample(range(BIG_B + 1, BIG_NCOLS), min(tail, L - 2))
        front = rng.sample([c for c in other if c < BIG_B], L - 2 - len(behind))
        row = {c: rng.choice(pick) for c in behind + front}
        row[BIG_A], row[BIG_B] = 2, 3
        cols = sorted(row)
        assert len(cols) == L
        ends.add(("a" if cols[L - 2] == BIG_A else "b" if cols[L - 2] == BIG_B else "other", cols[-1] == BIG_B, L == 2))
        rows += [dict(row), dict(row)]
    # what the row-end store overwrites (a, b, neither), with b last and not last, and rows of two entries
    assert {("a", True, True), ("a", True, False), ("b", False, False), ("other", True, False), ("other", False, False)} <= ends, ends
    for _ in range(420):
        row = {c: rng.choice(pick) for c in rng.sample(other, 10)}
        rows += [dict(row), dict(row)]
    rng.shuffle(rows)                                         # whichever rows a wave gets, their lengths are a random draw of 2..9
    return rows


@pytest.fixture(scope="module")
def big():
    rows = _big_matrix()
    M, ties = top_level(rows)
    assert M == 600 and [k[:2] for k in ties] == [(BIG_A, BIG_B)], (M, ties)      # the first step rewrites the 600 rows
    return _tie_case(rows, BIG_NCOLS, BIG_SEED0, BIG_NSEEDS)


@pytest.mark.parametrize("env", [{}, {"PLO_BIG_FWIN": "128"}, {"PLO_BIG_WIDE": "1"}, {"PLO_BIG_IDKEYS": "1"},
                                 {"PLO_BIG_WIDE": "1", "PLO_BIG_IDKEYS": "1", "PLO_BIG_FWIN": "128"}],
                         ids=lambda e: "-".join("%s%s" % (k[8:], v) for k, v in sorted(e.items())) or "default")
def test_row_end_store(hip, big, env):
    csr, want = big
    got, cnt = _run(csr, BIG_SEED0, BIG_NSEEDS, env)
    assert got == want
    assert cnt["candidates"] == BIG_NSEEDS and cnt["eager_refits"] == 0 and cnt["rows_searched"] >= BIG_NSEEDS * 600, cnt
    assert cnt["merge_groups"] > 0, cnt                      # deferred updates: the flat sweep is the one that ran
    if "PLO_BIG_FWIN" in env:
        # thread 0's wave, first step: 75 rows in batches of 64 and 11; the 64 are a random draw of the 600 lengths 2..9 (mean 5.5,
        # deviation 2.3: 352 entries, deviation 18), so more than 2 x 128 entries: at least two further windows
        assert cnt["extra_sweep_windows"] >= BIG_NSEEDS * 2, cnt
    else:
        assert cnt["extra_sweep_windows"] == 0, cnt


def test_merge_scans_one_partition_per_group(hip, big):
    csr, want = big
    got, cnt = _run(csr, BIG_SEED0, BIG_NSEEDS, {"PLO_BIG_LGRP": "64"})
    assert got == want
    merges = cnt["full_scans"] - BIG_NSEEDS                   # (the first scan of a candidate only chooses the window)
    assert cnt["eager_refits"] == 0 and merges >= BIG_NSEEDS and cnt["merge_groups"] >= 2 * merges, cnt


def test_merge_scans_forced_merges(hip, big):
    csr, want = big
    got, cnt = _run(csr, BIG_SEED0, BIG_NSEEDS, {"PLO_BIG_LOGTRIG": "2000"})
    assert got == want
    # a filler pair alone shrinks from 10 entries to 2 in steps that rewrite its two rows: some 36 distinct (column, ratio) entries,
    # three records each, times 420 pairs: above 40,000 records per candidate, twenty times the trigger; 4 is a floor

    assert cnt["eager_refits"] == 0 and cnt["merge_groups"] > 0 and cnt["forced_merges"] >= BIG_NSEEDS * 4, cnt
