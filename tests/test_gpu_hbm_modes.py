"""The value-table modes of the HBM-resident kernel (plo_cse_big.hip: mode 1, value table in LDS; mode 0, in global memory) where the rest of
the suite does not take them: at moduli that are no Mersenne primes -- Barrett's reduction in every ratio, Fermat's inverse in the flush above
2^20, the single-ratio aggregation entry where the dual one does not fit, pair keys of up to all 48 bits -- and on matrices whose pair triples
repeat, so that the steps, not the naive count, decide the result.

The cases are those of tests/hbm_modes_cases.py (tests/test_hbm_modes_cases_host.py proves what they are on the host).  Each runs against the
literal oracle, (adds, muls) equal seed by seed, once with the plan's own choice between deferred updates and the eager pair table and once
with PLO_BIG_EAGER=1, and asserts through plo_cse_plan_hbm_info that the plan is the one the case is here for."""
import pytest

import hbm_modes_cases as H
from plo_testlib import OracleMatrix

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
RUN = [c for c in H.CASES if not c.refused]


def _plan(case, monkeypatch, eager):
    from plinopt_amd import CSEPlan
    if eager:
        monkeypatch.setenv("PLO_BIG_EAGER", "1")
    if case.knob:
        monkeypatch.setenv(case.knob, "1")
    rp, c, v = case.csr()
    plan = CSEPlan(case.m, case.n, rp, c, v, case.p, hbm=True)
    assert plan.is_hbm
    info = plan.hbm_info()
    assert info == case.plan_info(eager=eager)
    assert {k: info[k] for k in case.info if k not in ("defer", "pbits") or not eager} == {k: x for k, x in case.info.items() if k not in ("defer", "pbits") or not eager}
    return plan, info


@pytest.mark.parametrize("eager", [False, True], ids=["default", "eager"])
@pytest.mark.parametrize("case", RUN, ids=repr)
def test_costs_equal_the_oracle(hip, monkeypatch, case, eager):
    plan, info = _plan(case, monkeypatch, eager)
    got = plan.cost_many(seed0=case.seed0, n=H.NSEEDS)
    print(case.name, "eager" if eager else "default", info, got, H.oracle_costs(case))
    assert got == H.oracle_costs(case)
    cnt = plan.hbm_counters()
    assert cnt["steps"] >= H.NSEEDS and cnt["candidates"] == H.NSEEDS
    assert cnt["eager_refits"] == 0 and plan.hbm_info() == info              # the plan that was asserted is the one that ran
    plan.close()


@pytest.mark.parametrize("eager", [False, True], ids=["default", "eager"])
@pytest.mark.parametrize("name", H.ARGMIN)
def test_search_argmin(hip, monkeypatch, name, eager):
    """(e) the minimum under the three cost orders, ties to the smallest seed"""
    case = H.BY_NAME[name]
    plan, info = _plan(case, monkeypatch, eager)
    rp, c, v = case.csr()
    M = OracleMatrix(case.m, case.n, rp, c, v, case.p)
    for cost_mode in (0, 1, 2):
        assert plan.search(case.seed0, H.ARGMIN_SEEDS, cost_mode=cost_mode) == M.search(case.seed0, H.ARGMIN_SEEDS, cost_mode=cost_mode, nthreads=8)
    assert plan.hbm_counters()["steps"] >= H.ARGMIN_SEEDS
    plan.close()


def test_one_column_too_many_for_a_30_bit_residue_is_refused(hip):
    """(g) a column bound of 513 beside a 30-bit residue does not fit the 48-bit pair key, and 48 values get no ratio identifiers: refused when
    the plan is made, with the reason.  (g-512-columns and g-513-columns-32-values, above, are the two neighbours that are taken.)"""
    from plinopt_amd import CSEPlan, capi
    case = H.BY_NAME["g-513-columns"]
    rp, c, v = case.csr()
    with pytest.raises(capi.PloError, match=case.refused) as e:
        CSEPlan(case.m, case.n, rp, c, v, case.p, hbm=True)
    assert e.value.code == capi.PLO_E_CAPACITY


def test_hbm_info_is_for_hbm_plans(hip):
    from plinopt_amd import CSEPlan, capi
    plan = CSEPlan(2, 2, [0, 2, 4], [0, 1, 0, 1], [1, 1, 1, H.P21 - 1], H.P21)
    assert not plan.is_hbm
    with pytest.raises(capi.PloError) as e:
        plan.hbm_info()
    assert e.value.code == capi.PLO_E_ARG
    plan.close()
