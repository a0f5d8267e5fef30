"""The sweep of plo::cse_big_kernel where its addressing can go wrong, against the LITERAL oracle.

The kernels address a candidate's workspace slice as one base plus 32-bit byte offsets (plo::WsArr), with the large table / store
region last behind a pointer of its own, and kernels with 64-bit offsets for slices whose front region passes 4 GiB.  The flat
sweep (mode 2 with deferred updates) takes the entries of a wave's next 64 rows as ONE sequence, 64 per trip, in windows of
`fwin` entries, requests entries two trips ahead and runs a trip loop unrolled three times.  One synthetic matrix drives every
edge of that, small enough for the oracle (seconds, computed once per module) and large enough for the plan to take the
deferred updates (some 24,000 distinct triples of frequency >= 2; `merge_groups` > 0 below says that it did):

  rows come in identical pairs (every triple has frequency >= 2), values from {+-1, +-2, 3}: at most 32 values, so mode 2;
  group g has f_g rows of L_g entries that share a two-column prefix (columns of its own, one ratio), f_g a multiple of 8: the
  step that takes the prefix rewrites f_g rows, every one of the 8 waves gets f_g / 8 of them, and -- all rows of a group having
  the same length, whatever order the row search found them in -- a wave's sequence is T = (f_g / 8) L_g entries:

    f_g x L_g   rows per wave   T                           what it reaches
    640 x 8     80              512 + 128 (two batches)     more than 512 rows in a step: a wave takes a SECOND batch of 64 rows
    320 x 8     40              320                         5 trips
    256 x 8     32              256                         4 trips
    192 x 8     24              192                         3 trips
    128 x 8     16              128                         2 trips
     64 x 8      8               64                         1 trip; the sequence ends exactly on the 64-entry boundary (the
                                                            mark of the last row's end is bit 0 of the NEXT trip's word)
     56 x 9      7               63                         the sequence ends at entry 63 of 64 (bit 63 of the trip's word)
      8 x 2      1                2                          rewritten rows of exactly two entries, both removed: the new
                                                            column's entry lands at position 0 of the row

  With fwin = 2048 (default) every sequence above is one window of 1..8 trips; PLO_BIG_FWIN=320 cuts them into windows of at
  most 5 trips (1, 2, 3, 4 and 5 trips all occur: 63 -> 1, 128 -> 2, 192 -> 3, 256 -> 4, 320 -> 5, 512 -> 5 + 3), PLO_BIG_FWIN=128
  into windows of 2 trips and of 1 (192 -> 2 + 1): the three exits of the unrolled loop, and the requests of trips t + 1 and
  t + 2 past a window's last trip, which may only touch the `safe` word.  After its prefix step a group goes on with thousands
  of steps that rewrite two rows of 7..3 entries.

Every run must give the oracle's (adds, muls) seed by seed; `hbm_counters()` must show steps and searched rows (a step rewrites
at least two rows: its triple has frequency >= 2 -- there is no counter of rewritten rows), and for the flat sweep further
windows (`extra_sweep_windows`, which only the flat sweep counts).
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
GROUPS = ((640, 8), (320, 8), (256, 8), (192, 8), (128, 8), (64, 8), (56, 9), (8, 2))
KNOBS = ("PLO_BIG_FWIN", "PLO_BIG_EAGER", "PLO_BIG_NORID", "PLO_BIG_VT_GLOBAL", "PLO_BIG_WIDE")


def _matrix():
    rng = random.Random(11)
    ncols = 420
    vals = [1, P - 1, 2, P - 2, 3]
    pick = [1, P - 1] * 4 + vals                             # mostly +-1
    rows = []
    pc = ncols
    for f, L in GROUPS:
        a, b = pc, pc + 1
        pc += 2
        va = rng.choice(vals)
        vb = va * rng.choice([1, P - 1, 2]) % P
        for _ in range(f // 2):
            row = {c: rng.choice(pick) for c in rng.sample(range(ncols), L - 2)}
            row[a], row[b] = va, vb
            rows += [dict(row), dict(row)]
    for _ in range(120):                                    # filler pairs of 10 entries: triples enough for the deferred plan
        row = {c: rng.choice(pick) for c in rng.sample(range(ncols), 10)}
        rows += [dict(row), dict(row)]
    return len(rows), pc, rows


@pytest.fixture(scope="module")
def case():
    """the matrix in CSR and the oracle's costs of seeds 1..8, computed once"""
    m, n, rows = _matrix()
    rp, c, v = synth.to_csr(rows, P)
    M = OracleMatrix(m, n, rp, c, v, P)
    want = tuple(M.cost_many(seed0=SEED0, nseeds=NSEEDS, nthreads=8))
    return (m, n, rp, c, v), want


def _run(csr, env=None, search_mode=None):
    from plinopt_amd import CSEPlan
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(env or {})
        m, n, rp, c, v = csr
        plan = CSEPlan(m, n, rp, c, v, P, hbm=True)           # PLO_PLAN_HBM
        assert plan.is_hbm
        got = plan.cost_many(seed0=SEED0, n=NSEEDS) if search_mode is None else plan.search(SEED0, NSEEDS, cost_mode=search_mode)
        cnt = plan.hbm_counters()
        plan.close()
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    print("HBM counters %s: %s" % (env or "default", cnt))
    return got, cnt


def _swept(cnt):
    """steps were made (the prefix steps at least: their triples are the only ones of their frequencies) and rows searched: every
    step rewrites >= 2 rows, so no case passes without entering the sweep.  (The counters are those of the LAST launch: a search may
    end with a launch of fewer candidates than it was asked for.)"""
    return cnt["candidates"] >= 1 and cnt["steps"] >= cnt["candidates"] * len(GROUPS) and cnt["rows_searched"] >= 2 * cnt["steps"] and cnt["eager_refits"] == 0


def test_flat_sweep_default_window(hip, case):
    csr, want = case
    got, cnt = _run(csr)
    assert got == want
    assert _swept(cnt), cnt
    assert cnt["merge_groups"] > 0, cnt                      # deferred updates: the flat sweep is the one that ran
    assert cnt["extra_sweep_windows"] == 0, cnt              # no sequence is longer than 2048 entries


@pytest.mark.parametrize("fwin", [128, 320, 64])
def test_flat_sweep_windows_of_one_to_five_trips(hip, case, fwin):
    csr, want = case
    got, cnt = _run(csr, {"PLO_BIG_FWIN": str(fwin)})
    assert got == want
    assert _swept(cnt) and cnt["merge_groups"] > 0, cnt
    # thread 0's wave, per candidate: the 640-row step alone has 512 + 128 entries in two batches
    assert cnt["extra_sweep_windows"] >= NSEEDS * ((512 + fwin - 1) // fwin - 1 + (128 + fwin - 1) // fwin - 1), cnt


@pytest.mark.parametrize("knob", ["PLO_BIG_EAGER", "PLO_BIG_NORID", "PLO_BIG_VT_GLOBAL"])
def test_other_kernel_modes(hip, case, knob):
    """the eager table (the region with a pointer of its own) and the two-rows sweep of the other two modes"""
    csr, want = case
    got, cnt = _run(csr, {knob: "1"})
    assert got == want
    assert _swept(cnt), cnt
    assert cnt["extra_sweep_windows"] == 0, cnt              # not the flat sweep
    if knob == "PLO_BIG_EAGER":
        assert cnt["merge_groups"] == 0, cnt


@pytest.mark.parametrize("env", [{}, {"PLO_BIG_FWIN": "128"}, {"PLO_BIG_EAGER": "1"}, {"PLO_BIG_NORID": "1"}, {"PLO_BIG_VT_GLOBAL": "1"},
                                 {"PLO_BIG_VT_GLOBAL": "1", "PLO_BIG_EAGER": "1"}, {"PLO_BIG_NORID": "1", "PLO_BIG_EAGER": "1"}])
def test_wide_offsets(hip, case, env):
    """PLO_BIG_WIDE=1 takes the kernels with 64-bit offsets (the ones for slices whose front region passes 4 GiB): same costs"""
    csr, want = case
    got, cnt = _run(csr, dict(env, PLO_BIG_WIDE="1"))
    assert got == want
    assert _swept(cnt), cnt


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_cost_modes(hip, case, mode):
    """the search's winner under each cost mode: the oracle's costs under the oracle's order (oracle/plo_oracle.c cost_key: sum then
    adds, adds then muls, sum only; ties to the smallest seed)"""
    csr, (adds, muls) = case
    key = {0: lambda a, u: (a + u, a), 1: lambda a, u: (a, u), 2: lambda a, u: (a + u, 0)}[mode]
    k = min(range(NSEEDS), key=lambda i: (key(adds[i], muls[i]), i))
    got, cnt = _run(csr, None, search_mode=mode)
    assert got == (adds[k], muls[k], SEED0 + k)
    assert _swept(cnt), cnt
