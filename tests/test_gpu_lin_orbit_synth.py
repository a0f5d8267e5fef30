"""The in-place linear kernel (plo_lin.hip, with t_linear<LIN_X> and t_simplify of plo_tril.hip) and the orbit kernel
(plo_orbit.hip) on the synthetic edge cases of tests/synth.py: empty rows, rows of 64 entries, 129 rows, column 16381, one
wave per workgroup and programs near the 160 KiB of LDS for the first; dimensions 1, 9 and 16, 1 / 2 / 4 waves per workgroup,
composite moduli and moduli next to 2^31, entries that vanish modulo the modulus and Q inputs just under the int64 bound
for the second.  Per-seed counts are bit-exact against tests/golden/lin_synth_costs.json and orbit_synth_costs.json (the
literal oracles tests/lin_oracle.py and tests/orbit_oracle.py); the named refusal cases raise the header's code and nothing
else is refused; the searches on tie-heavy inputs return the golden's argmin; the sharded searches equal one device."""
import json
import os

import pytest

import lin_oracle
import synth
from plo_testlib import GOLDEN

pytestmark = pytest.mark.gpu

LIN_GOLD = json.load(open(os.path.join(GOLDEN, "lin_synth_costs.json")))
ORB_GOLD = json.load(open(os.path.join(GOLDEN, "orbit_synth_costs.json")))
LIN = {c.name: c for c in synth.lin_cases()}
ORB = {c.name: c for c in synth.orbit_cases()}
LIN_TIE = {c.name: c for c in synth.lin_tie_cases()}
ORB_TIE = {c.name: c for c in synth.orbit_tie_cases()}
LIN_FAMILIES = sorted({e["family"] for e in LIN_GOLD["cases"]} - {"refuse"})
ORB_FAMILIES = sorted({e["family"] for e in ORB_GOLD["cases"]} - {"refuse"})


def code(name):
    from plinopt_amd import capi
    return getattr(capi, name)


def lin_plan(c):
    from plinopt_amd import LinPlan
    return LinPlan(*synth.qcsr(c.m, c.n, c.ent))


def orbit_args(c):
    return [synth.qcsr(*M) for M in (c.L, c.R, c.P)]


def orbit_plan(c):
    from plinopt_amd import OrbitPlan
    return OrbitPlan(*orbit_args(c), modulus=c.modulus, measure=c.measure)


def scored(plan, e):
    """the plan's outputs for the entry's seeds: one explicit list, or the (seed0, n) runs whose last ends on BASE_SEED"""
    if e["mode"] == "list":
        return plan.cost_many(e["seeds"])
    assert e["seeds"] == synth.SEEDS_RUNS
    return [x for s0, n in synth.SEED_RUNS for x in plan.cost_many(seed0=s0, n=n)]


def check_family(gold, cases, family, make_plan, flat):
    from plinopt_amd import capi
    refused, seen = [], 0
    for e in gold["cases"]:
        if e["family"] != family:
            continue
        c = cases[e["name"]]
        assert c.sha256 == e["sha256"], e["name"]
        try:
            plan = make_plan(c)
        except capi.PloError as ex:
            refused.append((e["name"], ex.code))
            continue
        got = [flat(x) for x in scored(plan, e)]
        assert got == e["out"], "%s: first differing seed %s" % (e["name"], next(s for s, a, b in zip(e["seeds"], got, e["out"]) if a != b))
        seen += 1
    assert refused == [], "refused == 0 outside the named refusal cases"
    assert seen > 0


@pytest.mark.parametrize("family", LIN_FAMILIES)
def test_lin_cost_many_bit_exact(hip, family):
    check_family(LIN_GOLD, LIN, family, lin_plan, lambda x: list(x[0]) + list(x[1]))


@pytest.mark.parametrize("family", ORB_FAMILIES)
def test_orbit_cost_many_bit_exact(hip, family):
    check_family(ORB_GOLD, ORB, family, orbit_plan, list)


def test_families_cover_the_issue():
    assert LIN_FAMILIES == list("abcdefghi") and ORB_FAMILIES == list("abcdef")


def test_refusal_cases_raise_the_headers_code(hip):
    from plinopt_amd import capi
    n = 0
    for gold, cases, make_plan in ((LIN_GOLD, LIN, lin_plan), (ORB_GOLD, ORB, orbit_plan)):
        for e in gold["cases"]:
            if "refusal" not in e:
                continue
            assert sorted(e) == ["family", "name", "refusal", "sha256"]
            with pytest.raises(capi.PloError) as ex:
                make_plan(cases[e["name"]])
            assert ex.value.code == code(e["refusal"]), e["name"]
            n += 1
    assert n == 5


def test_orbit_canonical_under_a_modulus_is_density(hip):
    """family f: plo_orbit_plan_create_q scores by density under a modulus whatever `measure` says (include/plinopt_hip.h)"""
    from plinopt_amd import OrbitPlan
    fam = [e for e in ORB_GOLD["cases"] if e["family"] == "f"]
    assert len(fam) == 2
    for e in fam:
        c = ORB[e["name"]]
        assert c.modulus == 131071 and c.measure == synth.CANONICAL
        both = [[list(x) for x in scored(OrbitPlan(*orbit_args(c), modulus=c.modulus, measure=ms), e)] for ms in (synth.DENSITY, synth.CANONICAL)]
        assert both[0] == both[1] == e["out"], e["name"]
        assert all(o[0] == o[1] for o in e["out"])


@pytest.mark.parametrize("name", sorted(LIN_TIE))
def test_lin_search_on_ties_is_the_golden_argmin(hip, name):
    T = next(t for t in LIN_GOLD["tie"] if t["name"] == name)
    c = LIN_TIE[name]
    assert c.sha256 == T["sha256"]
    ops, s0, n = T["out"], T["seed0"], T["n"]
    plan = lin_plan(c)
    assert [x for a, b in plan.cost_many(seed0=s0, n=n) for x in list(a) + list(b)] == ops
    want = min((ops[6 * k + 3 * v], ops[6 * k + 3 * v + 1], s0 + k, v) for k in range(n) for v in (0, 1))
    assert sum((ops[6 * k + 3 * v], ops[6 * k + 3 * v + 1]) == want[:2] for k in range(n) for v in (0, 1)) > 1, "no tie in the golden"
    (a, s, r), seed, var = plan.search(s0, n)
    assert (a, s, seed, var) == want
    assert r == ops[6 * (seed - s0) + 3 * var + 2]
    # the incumbent rule of lin_oracle.search (:613, :637-641): the loop's best is kept only when strictly better.  The device
    # API returns the loop's best and leaves the incumbent to its caller, so this applies the rule to the device's answer;
    # the tool's own implementation of it is held to T["search"] in tests/test_synth_golden.py
    base = tuple(T["base"][:3])
    final = ((a, s, r), seed, var) if lin_oracle.better((a, s, r), base) else (base, lin_oracle.BASE_SEED, 0)
    assert [list(final[0]), final[1], final[2]] == T["search"]


@pytest.mark.parametrize("name", sorted(ORB_TIE))
def test_orbit_search_on_ties_is_the_golden_argmin(hip, name):
    T = next(t for t in ORB_GOLD["tie"] if t["name"] == name)
    c = ORB_TIE[name]
    assert c.sha256 == T["sha256"] and (c.modulus, c.measure) == (T["modulus"], T["measure"])
    o, s0, n = T["out"], T["seed0"], T["n"]
    plan = orbit_plan(c)
    assert [x for t in plan.cost_many(seed0=s0, n=n) for x in t] == o
    want = min((o[3 * j], o[3 * j + 1], o[3 * j + 2], s0 + j) for j in range(n))
    assert sum(tuple(o[3 * j:3 * j + 3]) == want[:3] for j in range(n)) > 1, "no tie in the golden"
    (cost, nnz, nno), seed = plan.search(s0, n)
    assert (cost, nnz, nno, seed) == want
    assert list(plan.cost_many([synth.BASE_SEED])[0]) == T["base"]


@pytest.mark.parametrize("name", ["lin_g_rat", "lin_b_12of24_0-5-6-11_unit"])
def test_lin_search_multi_equals_one_device(hip, name):
    from plinopt_amd import lin_search_multi
    c = LIN[name]
    one = lin_plan(c).search(3, 301)
    for nd in (1, 2, 3):
        got, st = lin_search_multi(*synth.qcsr(c.m, c.n, c.ent), 3, 301, [0] * nd)
        assert got == one, (name, nd)
        assert st["candidates"] == 301


@pytest.mark.parametrize("name", ["orbit_a_9x9x9_r65", "orbit_c_mod15_10x16x9"])
def test_orbit_search_multi_equals_one_device(hip, name):
    from plinopt_amd import orbit_search_multi
    c = ORB[name]
    one = orbit_plan(c).search(3, 301)
    for nd in (1, 2, 3):
        got, st = orbit_search_multi(*orbit_args(c), c.modulus, c.measure, 3, 301, [0] * nd)
        assert got == one, (name, nd)
        assert st["candidates"] == 301
