"""Edge-shape parity of the CSE measure of the orbit search (plo::orbit_cse_kernel, plo_orbit_cse.hip; host side orbit_cse_layout,
orbit_cse_size and plo_orbit_plan_create_cse of plo_capi.hip) against the literal oracle tests/orbit_cse_oracle.py on the inputs
of tests/orbit_cse_cases.py: the 64-lanes-per-row path of the image build (33 to 64 columns, rows of exactly 64 entries, 64 rows),
the entries-only restore between the Optimizer runs (PLO_ORBIT_CSE_KEEP=0), waves that score more than one candidate, the PLUQ
and Householder draws at 64 columns, and the reasons of the four refusals.  (cost, nnz, nno) are integers: every comparison is
exact.  No accepted case may be refused: the images are tiny (tests/test_orbit_cse_cases_host.py has their sizes)."""
import functools
import os

import pytest

import orbit_action_oracle as A
import orbit_cse_cases as cc
import orbit_cse_oracle as Z
import orbit_oracle as O
import synth
from plo_testlib import DATA, read_sms

pytestmark = pytest.mark.gpu
BASE = cc.BASE
LDS_CU = 160 * 1024                      # LDS of a CU


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(qcsr arguments, dense matrices, (m, k, n)) of a triple of data/"""
    mats, mkn = O.load(os.path.join(DATA, name))
    return [synth.qcsr(*read_sms(os.path.join(DATA, "%s_%s.sms" % (name, x)))) for x in "LRP"], mats, mkn


def short(c):
    return c.name.split("_", 2)[2]


def by_name(names):
    return pytest.mark.parametrize("name", names)


ACCEPTED = [short(c) for c in cc.accepted(cc.PRIMES[0])]
PRIME = pytest.mark.parametrize("p", cc.PRIMES)


def plan_of(args, p, sub, action=A.TRIANGULAR, cse_seed0=0):
    """the plan; a refusal is an error of the test that asks for it"""
    from plinopt_amd import ORBIT_CSE, OrbitPlan
    return OrbitPlan(*args, modulus=p, measure=ORBIT_CSE, action=action, sub=sub, cse_seed0=cse_seed0)


def same(got, want, seeds):
    assert got == want, next((s, a, b) for s, a, b in zip(seeds, got, want) if a != b)


# ------------------------------------------------------------------------------------------ 1. edge-shape parity
@PRIME
@by_name(ACCEPTED)
def test_edge_shapes_equal_the_oracle(hip, p, name):
    c = cc.named(p, name)
    plan = plan_of(cc.triple(c)[0], p, cc.SUB)                                # accepted: a PLO_E_CAPACITY here is a finding
    same(plan.cost_many(cc.SEEDS), cc.costs(c), cc.SEEDS)
    info = plan.info()
    print(name, p, info)
    assert info["relaunches"] == 0
    assert info["entry_bound"] == max(rows * cols for rows, cols in cc.dims(c))   # the hard bound: no candidate can outgrow the entries
    assert info["keeps_whole_image"] or max(info["table_slots"]) == 8192      # (entries alone only where a 64 KiB table and its copy do not fit)
    if max(c.mkn) <= 2:                                                       # (the 256 products of the sizing sample are cheap: factors of size 4)
        assert info["table_slots"] == cc.table_slots(c)
    else:
        assert all(64 <= s <= 8192 and s & (s - 1) == 0 for s in info["table_slots"])


# ------------------------------------------------------------------------------------------ 2. every action at 64 columns
@pytest.mark.parametrize("action", [A.PLUQ, A.HOUSEHOLDER], ids=["pluq", "householder"])
@pytest.mark.parametrize("p", [131071, 2147483629])
@by_name(["Lj_8x8x1_r2", "Lj_8x8x1_r2_dense", "rows_1x1x1_r64", "rows_1x1x1_r64_dense"])
def test_every_action_at_64_columns(hip, action, p, name):
    c = cc.named(p, name)
    plan = plan_of(cc.triple(c)[0], p, cc.SUB, action)
    same(plan.cost_many(cc.SEEDS), cc.costs(c, action=action), cc.SEEDS)
    assert plan.info()["relaunches"] == 0


# ------------------------------------------------------------------------------------------ 3. entries-only restore
def _restore_inputs(name):
    """(qcsr arguments, modulus, seeds, the oracle's costs for `sub`)"""
    if "x" in name.split("_")[0]:                                             # a fixture of data/
        args, mats, mkn = fixture(name)
        seeds = [BASE] + list(range(32))
        return args, 131071, seeds, lambda sub: _fixture_costs(name, tuple(seeds), sub)
    c = cc.named(131071, name)
    return cc.triple(c)[0], 131071, cc.SEEDS, lambda sub: cc.costs(c, sub=sub)


@functools.lru_cache(maxsize=None)
def _fixture_costs(name, seeds, sub):
    _, mats, mkn = fixture(name)
    return Z.costs(mats, mkn, list(seeds), 131071, sub, 0)[0]


@by_name(["2x2x2_7_Winograd", "3x3x3_23_58", "Lj_8x8x1_r2_dense", "rows_1x1x1_r64_dense"])
def test_entries_only_restore(hip, monkeypatch, name):
    """PLO_ORBIT_CSE_KEEP=0: between the runs the wave puts back the entries alone and makes masks and table again (oc_index);
    sub = 3 restores twice.  The same list as the oracle and as a plan that keeps the whole image."""
    args, p, seeds, want = _restore_inputs(name)
    monkeypatch.delenv("PLO_ORBIT_CSE_KEEP", raising=False)
    whole = plan_of(args, p, 3)
    assert whole.info()["keeps_whole_image"] is True
    monkeypatch.setenv("PLO_ORBIT_CSE_KEEP", "0")
    plan = plan_of(args, p, 3)
    assert plan.info()["keeps_whole_image"] is False
    got = plan.cost_many(seeds)
    same(got, want(3), seeds)
    same(got, whole.cost_many(seeds), seeds)
    assert plan.info()["relaunches"] == 0 and plan.info()["table_slots"] == whole.info()["table_slots"]
    if name in ("2x2x2_7_Winograd", "3x3x3_23_58"):
        assert want(3) != want(2) != want(1)                                  # each restored run decides some candidate's cost


def test_entries_only_restore_chosen_by_the_plan(hip, monkeypatch):
    """hP of (2,1,2) with r = 64 and a dense row: 4 rows of up to 64 entries, 8192 slots; the whole image and its copy do not fit
    LDS, so the plan keeps the entries without the knob.  Every seed's cost depends on the second or third run."""
    monkeypatch.delenv("PLO_ORBIT_CSE_KEEP", raising=False)
    c = cc.named(131071, "hP_2x1x2_r64_dense")
    want = cc.costs(c, sub=3)
    assert all(a != b for a, b in zip(want, cc.costs(c, sub=1))) and want != cc.costs(c, sub=2)
    plan = plan_of(cc.triple(c)[0], 131071, 3)
    info = plan.info()
    assert info["keeps_whole_image"] is False and info["table_slots"] == cc.table_slots(c) == (64, 64, 8192)
    same(plan.cost_many(cc.SEEDS), want, cc.SEEDS)
    assert plan.info()["relaunches"] == 0


@pytest.mark.parametrize("keep", ["0", "1"])
@by_name(["Lj_8x8x1_r2_dense", "rows_1x1x1_r64_dense"])
def test_one_run_keeps_no_copy(hip, monkeypatch, keep, name):
    """sub = 1: no copy at all, whatever the knob says"""
    c = cc.named(131071, name)
    monkeypatch.setenv("PLO_ORBIT_CSE_KEEP", keep)
    plan = plan_of(cc.triple(c)[0], 131071, 1)
    assert plan.info()["keeps_whole_image"] is (keep == "1")
    same(plan.cost_many(cc.SEEDS), cc.costs(c, sub=1), cc.SEEDS)


# ------------------------------------------------------------------------------------------ 4. several candidates per wave
_wino = {}


def winograd_costs(seeds, sub=2):
    """the oracle on 2x2x2_7_Winograd, p = 131071, per seed and once per process"""
    _, mats, mkn = fixture("2x2x2_7_Winograd")
    for s in seeds:
        if (s, sub) not in _wino:
            _wino[s, sub] = Z.cost3(mats, mkn, s, 131071, sub, 0)
    return [_wino[s, sub] for s in seeds]


@pytest.mark.parametrize("cap,keep", [(8192, "1"), (8192, "0"), (2048, "1")], ids=["whole-image", "entries", "whole-image-4-waves"])
def test_a_wave_scores_several_candidates(hip, monkeypatch, cap, keep):
    """Tables of 8192 slots leave one or two workgroups on a CU, so 2 x the resident waves + 3 candidates give waves a second
    and a third one: what a candidate leaves in the image, len, rs and the kept copy meets the next one.  With 2048 slots and
    the copy, a wave's region is a quarter of that: workgroups of several waves, each wave with neighbours in LDS."""
    import torch
    monkeypatch.setenv("PLO_ORBIT_CSE_CAP", str(cap))
    monkeypatch.setenv("PLO_ORBIT_CSE_KEEP", keep)
    plan = plan_of(fixture("2x2x2_7_Winograd")[0], 131071, 2)
    info = plan.info()
    assert info["table_slots"] == (cap, cap, cap) and info["keeps_whole_image"] is (keep == "1")
    assert cap == 8192 or info["waves_per_wg"] > 1
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 2 * cus * (LDS_CU // info["lds_bytes"]) * info["waves_per_wg"] + 3
    print("cap=%d keep=%s: %s, %d CUs, N = %d" % (cap, keep, info, cus, N))
    assert N <= 2100                                                          # (larger: the knob did not enlarge the plan)
    seeds = list(range(N)) + [BASE]
    want = winograd_costs(seeds)
    got = plan.cost_many(seeds)
    st = plan.last_stats
    print("grid %d x %d waves for %d candidates" % (st["grid"], info["waves_per_wg"], len(seeds)))
    first = st["grid"] * info["waves_per_wg"]
    assert first < N                                                          # at least one wave scored two candidates
    assert sum(a != b for a, b in zip(want[first:], winograd_costs(seeds[first:], 1))) >= 10   # whose cost the restored run decides
    same(got, want, seeds)
    best = min((c, s) for s, c in enumerate(want[:N]))                        # ties to the smaller seed
    assert plan.search(0, N) == best
    st = plan.last_stats
    assert st["grid"] * info["waves_per_wg"] < N and st["candidates"] == N
    assert plan.info()["relaunches"] == 0


# ------------------------------------------------------------------------------------------ 5. reasons of the refusals
@PRIME
@by_name([short(c) for c in cc.refused(cc.PRIMES[0])])
def test_refusals_name_their_quantity(hip, p, name):
    from plinopt_amd import ORBIT_DENSITY, OrbitPlan, capi
    c = cc.named(p, name)
    args = cc.triple(c)[0]
    with pytest.raises(capi.PloError) as e:
        plan_of(args, p, cc.SUB)
    assert e.value.code == capi.PLO_E_CAPACITY and "CSE measure: " + c.reason in str(e.value), e.value
    plan = OrbitPlan(*args, modulus=p, measure=ORBIT_DENSITY)                 # the limit is the CSE plan's own
    assert len(plan.cost_many([BASE, 0])) == 2
