"""plo::cse_big_kernel after the claimed-slot bitmap left the flat sweep and the compaction of the walked row list stopped looking
its list up again, against the LITERAL oracle, seed by seed (reference include/plinopt_optimize.inl:60-194, :237-312).

What changed and what each group of cases holds to it:

1. Flush without the bitmap.  The kernels with deferred updates and ratio identifiers (cse_big_kernel<2, true, ., .>) no longer keep
   a bit per claimed slot of the LDS aggregation table: in the flush a thread reads the key words of its 8 aligned pairs of slots
   (pair tid + u x 512, u = 0..7) and takes the slots that hold a key.  Three table sizes: PLO_BIG_AGGBITS=6, 32 pairs, one each for
   threads 0..31 (the bound on the pair index cuts every other read), the table fills and the rest of the step goes through the
   spill list; PLO_BIG_AGGBITS=8, 128 pairs, partly full; the default 2^13 slots, eight pairs per thread, where most pairs are empty
   and the small steps claim a single slot.
   Inputs: `4x4x4_49_156_P.sms` and synth.sweep(901, P, 220, 48, density=0.3, unit_frac=1.0) with the HBM family forced.  Both are
   too small for the deferred plan (size_big_deferred wants room for the records of a whole step in the log: some 10^4 triples of
   frequency >= 2), so they run the kernels that keep the slot LIST -- the other side of the change, which must stay as it was.
   The 128-row cut of 32x32x32_15096_L (tests/golden/l32cut_costs.json, costs by the literal oracle) does get the deferred plan --
   asserted here by `merge_groups` > 0, a counter only that plan moves -- and runs the new flush at all three sizes.
2. Merges.  The same inputs with the log trigger, the group size and the hot window as small as tests/test_gpu_merge_groups.py and
   tests/soak_hbm.py take them (PLO_BIG_LOGTRIG=2000, PLO_BIG_LGRP=64, PLO_BIG_HWIN=64: the plan clamps LGRP to >= 64 and the others
   to >= 1), so that a candidate of the cut makes dozens of forced merges and triples cross between the hot table and the store in
   both directions (a window of 64 triples is left after a few steps; every merge refills it from the store); once with
   PLO_BIG_IDKEYS=1 and once with PLO_BIG_WIDE=1 (the other instances of the deferred kernel).  Bound on the counter, as in
   test_gpu_merge_groups.py: a candidate of the cut logs ~10^5 records, far above 10 x 2000, so at least 10 forced merges each.
3. Compaction.  A step walks the shorter row list of its two columns and keeps the rows that still hold the list's column and do
   not lose it in this step; the list and its column are now carried across the search's barrier.  12 x 8: columns 0 and 1 share
   all 12 rows, rows 0-5 with ratio 1 and rows 6-11 with ratio 2.  Whichever of the two triples a seed takes first, the walked
   list (an input column's, 12 rows) keeps exactly the six rows of the other ratio; the second of the two then walks those six
   and keeps none.  The new column of rows 0-5 (a column >= n) lies in six rows, three of which hold column 2 with one value;
   column 2 lies in nine rows: the triple of column 2 and that new column, of frequency 3, is found by walking the CREATED
   column's list, which keeps three rows.  (A walked list that keeps EVERY row cannot occur: a step has at least two affected
   rows, they are in both lists, and they lose both columns.)
   A compaction that wrote to the wrong list or lost a live row shows in the costs -- the row would not be rewritten, and the
   kernel's own check of the rewritten rows against the triple's frequency would report it -- so the cases compare costs for 32
   seeds on the matrix and on 20 random matrices of the same shape, on the default kernel and on the eager, the mode 1 and the
   wide instances (the compaction is shared by all of them).
"""
import json
import os
import random

import pytest

import synth
from plo_testlib import DATA, GOLDEN, OracleMatrix, l32_cut, l32_rows

pytestmark = pytest.mark.gpu
P = 131071
KNOBS = ("PLO_BIG_AGGBITS", "PLO_BIG_LOGTRIG", "PLO_BIG_LGRP", "PLO_BIG_HWIN", "PLO_BIG_IDKEYS", "PLO_BIG_WIDE", "PLO_BIG_EAGER", "PLO_BIG_NORID")
NSMALL = 8          # seeds per run on the two small inputs
NCUT = 6            # seeds per run on the cut
SEED0 = 21


def _run(csr, seed0, n, env=None, hbm=True):
    """costs and counters of seeds seed0 .. seed0 + n - 1 with the knobs of `env` set (the plan reads them when it is built)"""
    from plinopt_amd import CSEPlan
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(env or {})
        m, nn, rp, c, v = csr
        plan = CSEPlan(m, nn, rp, c, v, P, hbm=hbm)
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


@pytest.fixture(scope="module")
def small(hip):
    """the two small inputs with the oracle's costs of seeds SEED0 .. SEED0 + NSMALL - 1 (computed once)"""
    out = {}
    M = OracleMatrix.from_sms(os.path.join(DATA, "4x4x4_49_156_P.sms"), P)
    out["4x4x4_P"] = ((M.m, M.n, M.rowptr, M.col, M.val), tuple(M.cost_many(seed0=SEED0, nseeds=NSMALL, nthreads=8)))
    m, n, rows = synth.sweep(901, P, 220, 48, density=0.3, unit_frac=1.0)
    rp, c, v = synth.to_csr(rows, P)
    M = OracleMatrix(m, n, rp, c, v, P)
    out["sweep901"] = ((m, n, rp, c, v), tuple(M.cost_many(seed0=SEED0, nseeds=NSMALL, nthreads=8)))
    return out


@pytest.fixture(scope="module")
def cut(hip):
    """the 128-row cut of 32x32x32_15096_L and its goldens for seeds 1 .. NCUT"""
    G = json.load(open(os.path.join(GOLDEN, "l32cut_costs.json")))
    _, _, rows = l32_rows(P)
    csr = l32_cut(G["row_lo"], G["row_hi"], P, rows)
    assert len(csr[3]) == G["nnz"] and G["seed0"] == 1
    return csr, (G["adds"][:NCUT], G["muls"][:NCUT])


AGG = [{"PLO_BIG_AGGBITS": "6"}, {"PLO_BIG_AGGBITS": "8"}, {}]
AGG_IDS = ["64_slots", "256_slots", "default"]
MERGE = {"PLO_BIG_LOGTRIG": "2000", "PLO_BIG_LGRP": "64", "PLO_BIG_HWIN": "64"}


# ------------------------------------------------------------------------------------------------ 1. the flush
@pytest.mark.parametrize("env", AGG, ids=AGG_IDS)
@pytest.mark.parametrize("name", ["4x4x4_P", "sweep901"])
def test_flush_on_the_small_inputs(small, name, env):
    csr, want = small[name]
    got, cnt = _run(csr, SEED0, NSMALL, env)
    assert got == want
    assert cnt["candidates"] == NSMALL


@pytest.mark.parametrize("env", AGG, ids=AGG_IDS)
def test_flush_without_the_bitmap_on_the_cut(cut, env):
    csr, want = cut
    got, cnt = _run(csr, 1, NCUT, env, hbm=False)
    assert got == want
    assert cnt["eager_refits"] == 0 and cnt["merge_groups"] > 0, cnt          # the deferred plan: the kernels whose flush changed
    if env.get("PLO_BIG_AGGBITS") == "6":
        assert cnt["spilled_pairs"] > 0, cnt        # a rewritten row of 48 entries alone has 46 entries to sum: with a second row's the 64 slots are gone


# ------------------------------------------------------------------------------------------------ 2. the merges
@pytest.mark.parametrize("inst", [{"PLO_BIG_IDKEYS": "1"}, {"PLO_BIG_WIDE": "1"}], ids=["idkeys", "wide"])
def test_forced_merges_on_the_cut(cut, inst):
    csr, want = cut
    got, cnt = _run(csr, 1, NCUT, dict(MERGE, **inst), hbm=False)
    assert got == want
    assert cnt["eager_refits"] == 0 and cnt["forced_merges"] >= NCUT * 10, cnt
    assert cnt["merge_groups"] >= cnt["forced_merges"], cnt


@pytest.mark.parametrize("inst", [{"PLO_BIG_IDKEYS": "1"}, {"PLO_BIG_WIDE": "1"}], ids=["idkeys", "wide"])
@pytest.mark.parametrize("name", ["4x4x4_P", "sweep901"])
def test_merge_knobs_on_the_small_inputs(small, name, inst):
    csr, want = small[name]
    got, _ = _run(csr, SEED0, NSMALL, dict(MERGE, **inst))
    assert got == want


# ------------------------------------------------------------------------------------------------ 3. the compaction
def _compaction_rows():
    rows = []
    for i in range(12):
        r = {0: 1, 1: 1 if i < 6 else 2}
        if i < 3 or i >= 6:
            r[2] = 3 if i < 3 else i - 2              # column 2: nine rows; one value in rows 0-2 (a triple with the new column of rows 0-5), all different below
        r[3 + i % 5] = 1 if i % 2 else P - 1          # a little else, so that the candidates go on for some steps
        rows.append(r)
    return rows


def _check_compaction_matrix(rows):
    """the construction of the docstring, checked on the matrix"""
    both = [i for i, r in enumerate(rows) if 0 in r and 1 in r]
    assert len(rows) == 12 and max(max(r) for r in rows) == 7 and both == list(range(12))
    ratios = [r[1] * pow(r[0], -1, P) % P for r in rows]
    assert ratios[:6] == [1] * 6 and ratios[6:] == [2] * 6
    with2 = [i for i, r in enumerate(rows) if 2 in r]
    assert len(with2) == 9 and [i for i in with2 if i < 6] == [0, 1, 2] and {rows[i][2] for i in (0, 1, 2)} == {3}
    # (0, 1, 1) and (0, 1, 2) are the top level: no other triple reaches frequency 6
    cnt = {}
    for r in rows:
        it = sorted(r.items())
        for x in range(len(it)):
            for y in range(x + 1, len(it)):
                k = (it[x][0], it[y][0], it[y][1] * pow(it[x][1], -1, P) % P)
                cnt[k] = cnt.get(k, 0) + 1
    top = sorted(k for k, f in cnt.items() if f == max(cnt.values()))
    assert max(cnt.values()) == 6 and top == [(0, 1, 1), (0, 1, 2)], (max(cnt.values()), top)


@pytest.fixture(scope="module")
def compaction(hip):
    rows = _compaction_rows()
    _check_compaction_matrix(rows)
    cases = [rows]
    rng = random.Random(12 * 8)
    for _ in range(20):
        cases.append([{j: rng.choice([1, P - 1, 2]) for j in range(8) if rng.random() < 0.6} or {0: 1} for _ in range(12)])
    out = []
    for rows in cases:
        rp, c, v = synth.to_csr(rows, P)
        M = OracleMatrix(12, 8, rp, c, v, P)
        out.append(((12, 8, rp, c, v), tuple(M.cost_many(seed0=0, nseeds=32))))
    return out


@pytest.mark.parametrize("env", [{}, {"PLO_BIG_EAGER": "1"}, {"PLO_BIG_NORID": "1"}, {"PLO_BIG_WIDE": "1"}], ids=["default", "eager", "mode1", "wide"])
def test_compaction_of_the_walked_list(compaction, env):
    searched = 0
    for csr, want in compaction:
        got, cnt = _run(csr, 0, 32, env)
        assert got == want, csr
        searched += cnt["rows_searched"]
    assert searched > 0
