"""The kernel-method kernel (plo_kmethod.hip through plo_kernel_search) and the trilinear kernel (plo_tril.hip through
plo_tril_*) on the synthetic edge cases of tests/synth.py: 128 rows, 64 columns, 64 dependent rows and rank 64 at once, rows of
Dep of every group width, empty rows, eight moduli from 3 to 2^31 - 1 and 4 / 2 / 1 waves per workgroup for the first; 1, 63,
64, 65 and 129 rows, rows of 64 entries in each of A, B and T, the row forms of `-e`, variable 16381, the switch to one wave
per workgroup and programs near the 160 KiB of LDS for the second.  Per-seed counts are bit-exact against
tests/golden/kmethod_synth_costs.json and tril_synth_costs.json (the C oracle, oracle/plo_oracle.c and
oracle/plo_tril_oracle.c); the named refusal cases raise the header's code and nothing else is refused; `best` is the golden's
argmin under each cost mode; a block of restarts shares its first seed's decomposition; the trilinear search on tie-heavy
inputs returns the golden's argmin; the sharded searches equal one device."""
import json
import os

import pytest

import synth
from plo_testlib import GOLDEN

pytestmark = pytest.mark.gpu

KM_GOLD = json.load(open(os.path.join(GOLDEN, "kmethod_synth_costs.json")))
TRIL_GOLD = json.load(open(os.path.join(GOLDEN, "tril_synth_costs.json")))
KM = {c.name: c for c in synth.kmethod_cases()}
TRIL = {c.name: c for c in synth.tril_cases()}
TRIL_TIE = {c.name: c for c in synth.tril_tie_cases()}
KM_FAMILIES = sorted({e["family"] for e in KM_GOLD["cases"]} - {"refuse"})
TRIL_FAMILIES = sorted({e["family"] for e in TRIL_GOLD["cases"]} - {"refuse"})
KM_ENTRY = {e["name"]: e for e in KM_GOLD["cases"]}
TRIL_ENTRY = {e["name"]: e for e in TRIL_GOLD["cases"]}
_km_done, _tril_done = {}, {}


def code(name):
    from plinopt_amd import capi
    return getattr(capi, name)


def km_key(ops, seed, cost_mode=0):
    from plinopt_amd import cmp_op_count_key
    return cmp_op_count_key(ops[0], ops[1], cost_mode) + (seed,)


def km_runs(e):
    """the entry's seeds and counts cut into the (seed0, n) runs of synth.SEED_RUNS"""
    assert e["mode"] == "runs" and e["seeds"] == synth.SEEDS_RUNS
    at = 0
    for s0, n in synth.SEED_RUNS:
        yield s0, n, e["out"][at:at + n]
        at += n


def km_scored(name):
    """(counts per seed, best per run, stats of the last run) of plo_kernel_search on the case, once per session"""
    from plinopt_amd import kernel_search
    if name not in _km_done:
        c, got, bests, st = KM[name], [], [], None
        for s0, n, _ in km_runs(KM_ENTRY[name]):
            adds, muls, info, best, st = kernel_search(c.csr, c.p, s0, n)
            got += [[a, mu] + list(i) for a, mu, i in zip(adds, muls, info)]
            bests.append(best)
        _km_done[name] = (got, bests, st)
    return _km_done[name]


def tril_plan(c):
    from plinopt_amd import TrilPlan
    return TrilPlan(c.m, synth.tril_args(c), expanded=c.expanded)


def tril_scored(name):
    """(six counts per seed, the plan's stats) of plo_tril_cost_many on the case, once per session"""
    if name not in _tril_done:
        c, e = TRIL[name], TRIL_ENTRY[name]
        plan = tril_plan(c)
        if e["mode"] == "list":
            got = plan.cost_many(seeds=e["seeds"])
        else:
            assert e["seeds"] == synth.SEEDS_RUNS
            got = [x for s0, n in synth.SEED_RUNS for x in plan.cost_many(seed0=s0, n=n)]
        _tril_done[name] = ([list(a) + list(b) for a, b in got], plan.last_stats)
    return _tril_done[name]


def check_family(gold, cases, family, scored, after=None):
    from plinopt_amd import capi
    refused, seen = [], 0
    for e in gold["cases"]:
        if e["family"] != family:
            continue
        assert cases[e["name"]].sha256 == e["sha256"], e["name"]
        try:
            res = scored(e["name"])
        except capi.PloError as ex:
            refused.append((e["name"], ex.code))
            continue
        got = res[0]
        assert got == e["out"], "%s: first differing seed %s" % (e["name"], next(s for s, a, b in zip(e["seeds"], got, e["out"]) if a != b))
        if after:
            after(e, res)
        seen += 1
    assert refused == [], "refused == 0 outside the named refusal cases"
    assert seen > 0


def km_best_is_argmin(e, res):
    for (s0, n, out), best in zip(km_runs(e), res[1]):
        k = min(range(n), key=lambda k: km_key(out[k], s0 + k))
        assert best == (out[k][0], out[k][1], s0 + k), (e["name"], s0)


@pytest.mark.parametrize("family", KM_FAMILIES)
def test_kernel_search_bit_exact(hip, family):
    check_family(KM_GOLD, KM, family, km_scored, km_best_is_argmin)


@pytest.mark.parametrize("family", TRIL_FAMILIES)
def test_tril_cost_many_bit_exact(hip, family):
    check_family(TRIL_GOLD, TRIL, family, tril_scored)


def test_families_cover_the_issue():
    assert KM_FAMILIES == list("abcdef") and TRIL_FAMILIES == list("abcde")


def test_refusal_cases_raise_the_headers_code(hip):
    from plinopt_amd import capi, kernel_search
    n = 0
    for gold, cases, run in ((KM_GOLD, KM, lambda c: kernel_search(c.csr, c.p, 0, 8)), (TRIL_GOLD, TRIL, tril_plan)):
        for e in gold["cases"]:
            if "refusal" not in e:
                continue
            assert sorted(e) == ["family", "name", "refusal", "sha256"]
            with pytest.raises(capi.PloError) as ex:
                run(cases[e["name"]])
            assert ex.value.code == code(e["refusal"]), e["name"]
            n += 1
    assert n == 13


def test_kernel_search_waves_per_workgroup(hip):
    """4, 2 and 1 waves per workgroup all launch: the choice follows from the host layout and the 160 KiB of a CU"""
    waves = {e["name"]: km_scored(e["name"])[2]["waves_per_wg"] for e in KM_GOLD["cases"] if "refusal" not in e}
    assert set(waves.values()) == {1, 2, 4}, waves
    assert waves["km_a_4x2"] == 4 and waves["km_a_128x64"] == 1


def test_tril_waves_per_workgroup(hip):
    """four waves per workgroup up to 64 KiB of LDS, one beyond: the plan's own choice equals the layout tests/synth.py restates"""
    seen = set()
    for e in TRIL_GOLD["cases"]:
        if "refusal" in e:
            continue
        st, c = tril_scored(e["name"])[1], TRIL[e["name"]]
        assert (st["waves_per_wg"], st["lds_bytes"]) == (c.waves, c.lds), e["name"]
        seen.add(st["waves_per_wg"])
    assert seen == {1, 4}


@pytest.mark.parametrize("name", ["km_e_mod101", "km_a_128x64"])
def test_kernel_search_cost_modes(hip, name):
    """`best` under each of the three orders of cmpOpCount, ties to the smallest seed (PLO_COST_SUM returns the sum in .adds)"""
    from plinopt_amd import capi, kernel_search
    c, e = KM[name], KM_ENTRY[name]
    for mode in (capi.COST_SUM_THEN_ADD, capi.COST_ADD_THEN_MUL, capi.COST_SUM):
        for s0, n, out in km_runs(e):
            k = min(range(n), key=lambda k: km_key(out[k], s0 + k, mode))
            want = (out[k][0] + out[k][1], 0, s0 + k) if mode == capi.COST_SUM else (out[k][0], out[k][1], s0 + k)
            assert kernel_search(c.csr, c.p, s0, n, cost_mode=mode, want_costs=False)[3] == want, (name, mode, s0)


def test_kernel_search_blocks_share_the_first_seeds_decomposition(hip):
    """per_block = 16 over 50 restarts: three blocks of 16 and a last one of 2"""
    from plinopt_amd import kernel_search
    B = KM_GOLD["per_block"]
    c = KM[B["name"]]
    s0, n, per = B["seed0"], B["n"], B["per_block"]
    assert (s0, n, per) == synth.KM_PER_BLOCK and n % per and B["seeds"] == list(range(s0, s0 + n, per))
    adds, muls, info, _, _ = kernel_search(c.csr, c.p, s0, n, per_block=per)
    for b, want in enumerate(B["out"]):
        assert [adds[b * per], muls[b * per]] + list(info[b * per]) == want, B["seeds"][b]
        assert all(list(info[k]) == want[2:] for k in range(b * per, min(n, (b + 1) * per))), B["seeds"][b]


@pytest.mark.parametrize("name", sorted(TRIL_TIE))
def test_tril_search_on_ties_is_the_golden_argmin(hip, name):
    T = next(t for t in TRIL_GOLD["tie"] if t["name"] == name)
    c = TRIL_TIE[name]
    assert c.sha256 == T["sha256"] and c.expanded == T["expanded"]
    ops, s0, n = T["out"], T["seed0"], T["n"]
    plan = tril_plan(c)
    assert [x for a, b in plan.cost_many(seed0=s0, n=n) for x in list(a) + list(b)] == ops
    want = min((ops[6 * k + 3 * v], ops[6 * k + 3 * v + 1], s0 + k, v) for k in range(n) for v in (0, 1))
    assert sum((ops[6 * k + 3 * v], ops[6 * k + 3 * v + 1]) == want[:2] for k in range(n) for v in (0, 1)) > 1, "no tie in the golden"
    (a, s, mul), seed, var = plan.search(s0, n)
    assert (a, s, seed, var) == want and mul == ops[6 * (seed - s0) + 3 * var + 2]
    assert [[a, s, mul], seed, var] == T["search"]


def test_kernel_search_multi_equals_one_device(hip):
    from plinopt_amd import kernel_search, kernel_search_multi
    c = KM["km_a_68x34"]
    one = kernel_search(c.csr, c.p, 3, 301, want_costs=False)[3]
    for nd in (1, 2, 3):
        got, st = kernel_search_multi(c.csr, c.p, 3, 301, [0] * nd)
        assert got == one, nd
        assert st["candidates"] == 301


def test_tril_search_multi_equals_one_device(hip):
    from plinopt_amd import tril_search_multi
    c = TRIL["tril_a_m65_rat"]
    one = tril_plan(c).search(3, 301)
    for nd in (1, 2, 3):
        got, st = tril_search_multi(c.m, synth.tril_args(c), 3, 301, [0] * nd, expanded=c.expanded)
        assert got == one, nd
        assert st["candidates"] == 301
