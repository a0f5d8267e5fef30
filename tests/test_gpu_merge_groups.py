"""The merge of the deferred updates (plo::defer_merge, pass B) with its knobs turned, against the LITERAL oracle.

Pass B sums every group of partitions in an LDS table: the records of a group are prefetched across its partitions and the table
is emptied by the scan that reads it.  The natural run of the two literal-oracle fixtures (tests/golden/l32cut_costs.json, rows of
48 and 288 entries; tests/golden/longrow_costs.json, rows of 461..627 entries) takes only the common path: groups of one to three
partitions and up to 3000 records, merges mostly when the top level falls out of the window.  The knobs force the others:

  PLO_BIG_LGRP=64      a partition with more than 64 records is a group of its own (the g == 0 -> 1 clamp, tot above lgrp, the
                       table sized by tot)
  PLO_BIG_LGRP=7000    groups of several partitions and of more than 4 x 512 records: the loads behind the prefetch run
  PLO_BIG_LOGTRIG=2000 a merge whenever the log holds 2000 records: dozens of forced merges per candidate, near-empty
                       partitions, groups of up to 64 partitions, lanes whose partition has no record
  PLO_BIG_HWIN=64      a window of 64 hot triples: the top level leaves it after a few steps
  PLO_BIG_HOTBITS=6    a hot table of 64 slots to begin with (see test_cut_small_initial_hot_table for what that can reach)

Every case must reproduce the goldens bit for bit (reference include/plinopt_optimize.inl:237-312 picks the same pair whatever
the order in which the merge stores its records), and the counters of plo_cse_plan_hbm_counters_ex ([10] forced_merges,
[11] merge_groups, [12] merge_loop_records) must show that the path was taken.

Bounds on the counters, from the construction and not from a run (merges = full_scans - candidates: the first scan of a candidate
only chooses the window on the plan's image):
  * LGRP=64: a partition of more than 64 records is a group of its own, and on both fixtures every partition holds hundreds of
    records at every merge (the plan makes a partition for every 640..1280 triples of the input).  So merge_groups is exactly
    merges x partitions, a power of two for each merge, and above the natural run's, whose groups take several partitions wherever
    they fit 3000 records.  (On the cut the natural groups are mostly single partitions already -- a partition and its share of
    the log come to ~2,300 records -- so "above" is all that can be said there; on the long rows it is 2.7 times.)
  * LGRP=7000: no more groups than the natural run, and the loads behind the prefetch run in every group of more than 4 x 512
    records; a merge sums tens of thousands of records in groups of up to 7000, so there are such groups whatever the partition sizes.
  * LOGTRIG=2000: a candidate of the cut logs three records or so for each rewritten entry of its > 600 steps, some 10^5 in all
    and far above 10 x 2000; every 2000 records force a merge: at least 10 forced merges per candidate, and that many more full
    scans than the natural run.
"""
import json
import os

import pytest

from plo_testlib import GOLDEN, l32_cut, l32_rows, longrow_matrix

pytestmark = pytest.mark.gpu
P = 131071
NSEEDS = 8
KNOBS = ("PLO_BIG_LGRP", "PLO_BIG_LOGTRIG", "PLO_BIG_HWIN", "PLO_BIG_HOTBITS")


def _run(csr, seed0, n, env=None):
    """costs and counters of seeds seed0 .. seed0 + n - 1 with the knobs of `env` set (the plan reads them when it is built)"""
    from plinopt_amd import CSEPlan
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(env or {})
        m, nn, rp, c, v = csr
        plan = CSEPlan(m, nn, rp, c, v, P)
        assert plan.is_hbm
        got = plan.cost_many(seed0=seed0, n=n)
        cnt = plan.hbm_counters()
        plan.close()
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    print("HBM counters %s: %s" % (env or "natural", cnt))
    return got, cnt


@pytest.fixture(scope="module")
def cut(hip):
    """the 128-row cut, its goldens for seeds 1..8 and the counters of its natural run"""
    G = json.load(open(os.path.join(GOLDEN, "l32cut_costs.json")))
    _, _, rows = l32_rows(P)
    csr = l32_cut(G["row_lo"], G["row_hi"], P, rows)
    assert len(csr[3]) == G["nnz"] and G["seed0"] == 1
    want = (G["adds"][:NSEEDS], G["muls"][:NSEEDS])
    got, cnt = _run(csr, 1, NSEEDS)
    assert got == want
    return csr, want, cnt


@pytest.fixture(scope="module")
def longrow(hip):
    """the long-row matrix, its goldens (seeds 1..4) and the counters of its natural run"""
    G = json.load(open(os.path.join(GOLDEN, "longrow_costs.json")))
    csr = longrow_matrix(P)
    assert len(csr[3]) == G["nnz"] and G["seed0"] == 1
    want = (G["adds"], G["muls"])
    got, cnt = _run(csr, 1, len(G["adds"]))
    assert got == want
    return csr, want, cnt


def test_cut_natural_run(cut):
    _, _, cnt = cut
    assert cnt["candidates"] == NSEEDS and cnt["eager_refits"] == 0
    assert cnt["full_scans"] >= 2 * NSEEDS                     # the first window of a candidate and at least one merge
    assert cnt["merge_groups"] >= cnt["full_scans"] - NSEEDS   # every merge sums at least one group


def _one_group_per_partition(cnt, ncand):
    merges = cnt["full_scans"] - ncand
    per = cnt["merge_groups"] // merges
    return cnt["merge_groups"] == per * merges and per >= 2 and per & (per - 1) == 0


def test_cut_one_partition_per_group(cut):
    csr, want, nat = cut
    got, cnt = _run(csr, 1, NSEEDS, {"PLO_BIG_LGRP": "64"})
    assert got == want
    assert cnt["eager_refits"] == 0 and cnt["full_scans"] == nat["full_scans"], (cnt, nat)
    assert cnt["merge_groups"] > nat["merge_groups"] and _one_group_per_partition(cnt, NSEEDS), (cnt, nat)


def test_cut_groups_beyond_the_prefetch(cut):
    csr, want, nat = cut
    got, cnt = _run(csr, 1, NSEEDS, {"PLO_BIG_LGRP": "7000"})
    assert got == want
    assert cnt["eager_refits"] == 0 and cnt["merge_loop_records"] > 0 and cnt["merge_groups"] < nat["merge_groups"], (cnt, nat)


def test_cut_merges_forced_by_the_log(cut):
    csr, want, nat = cut
    got, cnt = _run(csr, 1, NSEEDS, {"PLO_BIG_LOGTRIG": "2000"})
    assert got == want
    assert cnt["eager_refits"] == 0 and cnt["forced_merges"] >= NSEEDS * 10, cnt
    assert cnt["full_scans"] >= nat["full_scans"] + NSEEDS * 10, (cnt, nat)


def test_cut_forced_merges_small_window_and_single_partitions(cut):
    csr, want, nat = cut
    got, cnt = _run(csr, 1, NSEEDS, {"PLO_BIG_LOGTRIG": "2000", "PLO_BIG_HWIN": "64", "PLO_BIG_LGRP": "64"})
    assert got == want
    assert cnt["eager_refits"] == 0 and cnt["forced_merges"] >= NSEEDS * 10, cnt
    assert cnt["full_scans"] >= nat["full_scans"] + NSEEDS * 10, (cnt, nat)


def test_cut_small_initial_hot_table(cut):
    """PLO_BIG_HOTBITS=6 lowers only the FLOOR of the hot table's size.  Every merge sizes the table to at least 4 x window + 1024
    slots and a table that is half full forces a merge, so a hot table cannot fill up on this fixture and the repeat of the launch on
    a larger table (`eager_refits`, the counter that refit raises; tests/soak_hbm.py reaches it with random dense matrices) is out
    of this knob's reach: the counter stays 0, which is asserted, and the run is the natural one, merge for merge."""
    csr, want, nat = cut
    got, cnt = _run(csr, 1, NSEEDS, {"PLO_BIG_HOTBITS": "6"})
    assert got == want
    assert cnt["eager_refits"] == 0 and cnt["full_scans"] == nat["full_scans"] and cnt["merge_groups"] == nat["merge_groups"], (cnt, nat)


def test_longrow_natural_run(longrow):
    _, want, cnt = longrow
    assert cnt["candidates"] == len(want[0]) and cnt["eager_refits"] == 0
    assert cnt["merge_groups"] >= cnt["full_scans"] - len(want[0])


def test_longrow_one_partition_per_group(longrow):
    csr, want, nat = longrow
    got, cnt = _run(csr, 1, len(want[0]), {"PLO_BIG_LGRP": "64"})
    assert got == want
    assert cnt["eager_refits"] == 0 and cnt["full_scans"] == nat["full_scans"], (cnt, nat)
    assert cnt["merge_groups"] >= 2 * nat["merge_groups"] and _one_group_per_partition(cnt, len(want[0])), (cnt, nat)


def test_longrow_groups_beyond_the_prefetch(longrow):
    csr, want, nat = longrow
    got, cnt = _run(csr, 1, len(want[0]), {"PLO_BIG_LGRP": "7000"})
    assert got == want
    assert cnt["eager_refits"] == 0 and cnt["full_scans"] == nat["full_scans"], (cnt, nat)
    assert cnt["merge_loop_records"] > 0 and cnt["merge_groups"] < nat["merge_groups"], (cnt, nat)
