"""ProgramGen of the HBM-resident kernel family (plo_cse_big.hip: big_program_gen) against the literal CPU oracle, seed for
seed, on the smallest shapes at which its row-per-thread passes, the wave path of the long rows, the ordered compaction of
the Triangle columns and the Triangle applications can go wrong."""
import functools
import random

import pytest

import synth
from plo_testlib import OracleMatrix

pytestmark = pytest.mark.gpu
P = 131071


def _nonempty(rows):
    return [r if r else {0: 1} for r in rows]


def _case_a():
    """600 rows (512 threads take two rows each, the last round is partial); 698 CSE steps give 738 columns, so the compaction
    crosses thread chunks and wave boundaries; 32 Triangle columns."""
    m, n, rows = synth.sweep(901, P, 600, 40, density=0.3, unit_frac=0.5)
    return m, n, _nonempty(rows), 40, 6


def _case_b():
    """8 rows that CSE finds nothing in (40 random residues) reach FactorOutRows with ~120 entries: the wave path; the 120
    rows behind them take the per-thread path in the same launch."""
    rng = random.Random(5)
    vals = [rng.randint(2, P - 2) for _ in range(40)]
    rows = [{j: rng.choice(vals) for j in range(150) if rng.random() < 0.8} for _ in range(8)]
    m, n, more = synth.sweep(902, P, 120, 150, density=0.1, unit_frac=0.5)
    return 8 + m, n, _nonempty(rows + more), 3, 4


def _case_c():
    """273 Triangle columns and 53 applications for seed 7 (750 columns)."""
    rng = random.Random(9)
    vals = [1, P - 1, 2, P - 2, 3, 4, 6, P - 6, 12, pow(2, -1, P), pow(3, -1, P)]
    rows = [{j: rng.choice(vals) for j in range(24) if rng.random() < 0.5} for _ in range(700)]
    return 700, 24, _nonempty(rows), 7, 6


CASES = {"A": _case_a, "C": _case_c}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the case's CSR arrays and the oracle's per-seed costs, computed once"""
    m, n, rows, seed0, nseeds = CASES[name]()
    rp, c, v = synth.to_csr(rows, P)
    M = OracleMatrix(m, n, rp, c, v, P)
    return m, n, rp, c, v, seed0, nseeds, tuple(M.cost_many(seed0=seed0, nseeds=nseeds, nthreads=8))


def _gpu_costs(name):
    from plinopt_amd import CSEPlan
    m, n, rp, c, v, seed0, nseeds, ref = _reference(name)
    plan = CSEPlan(m, n, rp, c, v, P, hbm=True)
    try:
        assert plan.is_hbm
        return plan.cost_many(seed0=seed0, n=nseeds), ref
    finally:
        plan.close()


def test_more_rows_and_columns_than_threads(hip):
    got, ref = _gpu_costs("A")
    assert got == ref


# OracleMatrix.cost_many(seed0=3, nseeds=4) of case B.  The literal oracle rescans its pair map at every step and needs about half a
# minute per candidate on this input (70 k pairs), so its costs are frozen here as tests/test_gpu_config5.py freezes config 5's.
CASE_B_ORACLE = ([2261, 2273, 2256, 2272], [699, 701, 711, 696])


def test_rows_still_long_at_factor_out_rows(hip):
    from plinopt_amd import CSEPlan
    m, n, rows, seed0, nseeds = _case_b()
    assert max(len(r) for r in rows[:8]) > 64
    rp, c, v = synth.to_csr(rows, P)
    plan = CSEPlan(m, n, rp, c, v, P, hbm=True)
    try:
        assert plan.is_hbm
        assert plan.cost_many(seed0=seed0, n=nseeds) == CASE_B_ORACLE
    finally:
        plan.close()


@pytest.mark.parametrize("env", [None, "PLO_BIG_NORID", "PLO_BIG_EAGER"])
def test_triangle_applications(hip, monkeypatch, env):
    """ProgramGen is shared by all kernel instances: mode 2 (default), mode 1 (PLO_BIG_NORID) and the eager table."""
    if env:
        monkeypatch.setenv(env, "1")
    got, ref = _gpu_costs("C")
    assert got == ref


def _check(m, n, rows, seed0, nseeds):
    from plinopt_amd import CSEPlan
    rp, c, v = synth.to_csr(rows, P)
    M = OracleMatrix(m, n, rp, c, v, P)
    plan = CSEPlan(m, n, rp, c, v, P, hbm=True)
    try:
        assert plan.is_hbm
        assert plan.cost_many(seed0=seed0, n=nseeds) == tuple(M.cost_many(seed0=seed0, nseeds=nseeds)), rows
    finally:
        plan.close()


def test_all_unit_matrix_takes_the_early_return(hip):
    rng = random.Random(11)
    rows = _nonempty([{j: rng.choice([1, P - 1]) for j in range(12) if rng.random() < 0.4} for _ in range(40)])
    _check(40, 12, rows, 0, 8)


def test_far_fewer_rows_than_threads(hip):
    h, t = pow(2, -1, P), pow(3, -1, P)
    rows = [{0: 2, 1: 3, 3: 1, 4: h}, {0: 2, 2: P - 3, 4: 6}, {1: 3, 2: 3, 3: P - 1, 4: 12, 0: t}]
    _check(3, 5, rows, 0, 8)


def test_every_row_has_one_entry(hip):
    rng = random.Random(12)
    vals = [1, P - 1, 2, P - 2, 3, 6, pow(2, -1, P)]
    rows = [{rng.randrange(8): rng.choice(vals)} for _ in range(30)]
    _check(30, 8, rows, 0, 8)


def test_small_valued_matrices(hip):
    for s in range(20):
        m, n, rows = synth.small_valued(s, P)
        _check(m, n, rows, s, 8)
