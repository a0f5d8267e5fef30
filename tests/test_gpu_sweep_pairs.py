"""The flat sweep of plo::cse_big_kernel (mode 2, deferred updates) works on PAIRS of entries: a lane takes entries 2j, 2j + 1 of one
row -- one 8-byte load at a 4-byte aligned address, two shifted stores, two ratio-identifier lookups, ONE probe loop of the
aggregation table for both keys -- against the LITERAL oracle, on the matrix of tests/sweep_pairs_matrix.py: rows of 2, 3, 4, 5 and
of 65, 66, 127, 128, 129, 130 entries at even and odd start offsets, removed positions of either parity, next to each other inside
one pair and across two, first and last in the row, and a step of 600 rows (tests/test_sweep_pairs_cases_host.py asserts all that
from the construction).  Every run must give the oracle's (adds, muls) seed by seed, and `merge_groups` > 0 says that the plan took
the deferred updates, i.e. that the flat sweep is the one that ran.

PLO_BIG_FWIN=64 is the smallest window (32 pairs, half a trip); 192 is no multiple of 128 (96 pairs: the window's second trip is
half empty): the long rows then span windows and the windows end inside trips.  PLO_BIG_AGGBITS=6 leaves 64 slots in the aggregation table: keys find no room within their 8 pairs of
slots, for both entries of a lane's pair or for one of them, and those entries are retired directly (`spilled_pairs` > 0).
"""
import os

import pytest

import synth
from plo_testlib import OracleMatrix
from sweep_pairs_matrix import GROUPS, NCOLS, P, matrix

pytestmark = pytest.mark.gpu
NSEEDS = 8
SEED0 = 1
KNOBS = ("PLO_BIG_FWIN", "PLO_BIG_EAGER", "PLO_BIG_NORID", "PLO_BIG_IDKEYS", "PLO_BIG_VT_GLOBAL", "PLO_BIG_WIDE", "PLO_BIG_AGGBITS")


@pytest.fixture(scope="module")
def case():
    """the matrix in CSR and the oracle's costs of seeds 1..8, computed once"""
    rows, _, _ = matrix()
    rp, c, v = synth.to_csr(rows, P)
    M = OracleMatrix(len(rows), NCOLS, rp, c, v, P)
    want = tuple(M.cost_many(seed0=SEED0, nseeds=NSEEDS, nthreads=8))
    return (len(rows), NCOLS, rp, c, v), want


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
    """the groups' prefix steps at least, the 600 rows of the first among the rows searched, deferred updates (the flat sweep)"""
    return (cnt["candidates"] == NSEEDS and cnt["steps"] >= NSEEDS * len(GROUPS) and cnt["rows_searched"] >= NSEEDS * 600
            and cnt["eager_refits"] == 0 and cnt["merge_groups"] > 0)


def test_pairs(hip, case):
    csr, want = case
    got, cnt = _run(csr)
    assert got == want
    assert _swept(cnt), cnt
    assert cnt["spilled_pairs"] == 0, cnt                    # the aggregation table took every entry
    assert cnt["extra_sweep_windows"] == 0, cnt


@pytest.mark.parametrize("fwin", ["64", "192"])
def test_windows(hip, case, fwin):
    """windows of 32 pairs (half a trip) and of 96 (a trip and a half): rows of 33, 64 and 65 pairs span them"""
    csr, want = case
    got, cnt = _run(csr, {"PLO_BIG_FWIN": fwin})
    assert got == want
    assert _swept(cnt), cnt
    # thread 0's wave, first step: 64 rows of 2 to 9 entries are 64 to 320 pairs, 192 on average (deviation 10): more than 128,
    # i.e. at least five windows of 32 pairs or two of 96
    assert cnt["extra_sweep_windows"] >= NSEEDS * (4 if fwin == "64" else 1), cnt


def test_direct_retirement(hip, case):
    csr, want = case
    got, cnt = _run(csr, {"PLO_BIG_AGGBITS": "6"})
    assert got == want
    assert _swept(cnt), cnt
    assert cnt["spilled_pairs"] > 0, cnt


@pytest.mark.parametrize("env", [{"PLO_BIG_IDKEYS": "1"}, {"PLO_BIG_WIDE": "1"}], ids=lambda e: "+".join(sorted(k[8:].lower() for k in e)))
def test_other_instances(hip, case, env):
    csr, want = case
    got, cnt = _run(csr, env)
    assert got == want
    assert _swept(cnt), cnt
