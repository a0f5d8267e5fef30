"""The growth-factor measure of the orbit search on the MI355X (plo::orbit_growth_kernel<ACT> through
plo_orbit_plan_create_growth): per-seed (bits of the cost, nnz, nno) against tests/golden/orbit_growth_costs.json (the literal
oracle tests/orbit_growth_oracle.py), the two sides of the 2^53 proof, the argmin under (bits, nnz, nno, seed) with ties,
bin/orbiter -g --gpu 1 against --gpu 0 (winner line and written files byte for byte), and the codes of the refusals."""
import json
import os
import shutil
import subprocess

import pytest

import orbit_growth_cases as C
import orbit_growth_oracle as G
import synth
from plo_testlib import DATA, GOLDEN, ROOT, read_sms

pytestmark = pytest.mark.gpu

ORB = os.path.join(ROOT, "bin", "orbiter")
GOLD = json.load(open(os.path.join(GOLDEN, "orbit_growth_costs.json")))
CASES = {c.name: c for c in C.cases()}
ACT = {"triangular": 0, "pluq": 1}


def run(cmd, timeout=300):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout, r.stderr


def files(name, d=DATA):
    return [os.path.join(d, "%s_%s.sms" % (name, x)) for x in "LRP"]


def fixture_args(name):
    return [synth.qcsr(*read_sms(f)) for f in files(name)]


def case_args(c):
    return [synth.qcsr(*M) for M in (c.L, c.R, c.P)]


def scored(plan):
    """C.SEEDS both ways: an explicit list for the base seed and 2^40, a (seed0, n) run for 0 .. 63"""
    got = plan.growth_many([C.SEEDS[0]]) + plan.growth_many(seed0=0, n=64) + plan.growth_many(C.SEEDS[-1:])
    assert plan.growth_many(C.SEEDS) == got
    return [["%016x" % G.bits(c), nnz, nno] for c, nnz, nno in got]


def first_diff(got, want):
    return next((s, a, b) for s, a, b in zip(C.SEEDS, got, want) if a != b)


@pytest.mark.parametrize("entry", GOLD["fixtures"], ids=lambda e: e["name"])
def test_growth_many_bit_exact_on_fixtures(hip, entry):
    """fails without the feature: there is no OrbitGrowthPlan (the library lacks plo_orbit_plan_create_growth)"""
    from plinopt_amd import OrbitGrowthPlan, capi
    args = fixture_args(entry["name"])
    c = C.fixture_case(entry["name"])
    assert [C.growth_refusal(c, a) for a in (0, 1)] == ([None, None] if "DPS" not in entry["name"] else ["PLO_E_UNSUPPORTED"] * 2)
    for action, want in sorted(entry["out"].items()):
        if C.growth_refusal(c, ACT[action]):               # DPS-integral: outside the 2^53 proof; the host scores it (test_orbiter_growth_host.py)
            with pytest.raises(capi.PloError) as ex:
                OrbitGrowthPlan(*args, action=ACT[action])
            assert ex.value.code == capi.PLO_E_UNSUPPORTED
            continue
        got = scored(OrbitGrowthPlan(*args, action=ACT[action]))
        assert got == want, "%s %s: first differing seed %s" % ((entry["name"], action) + (first_diff(got, want),))


@pytest.mark.parametrize("entry", GOLD["cases"], ids=lambda e: e["name"])
def test_growth_many_bit_exact_on_edge_shapes(hip, entry):
    from plinopt_amd import OrbitGrowthPlan, capi
    c = CASES[entry["name"]]
    assert c.sha256 == entry["sha256"]
    for action, want in sorted(entry["out"].items()):
        if entry["refusal"][action]:                                   # (16 x 2 x 3 under PLUQ: outside the proof)
            with pytest.raises(capi.PloError) as ex:
                OrbitGrowthPlan(*case_args(c), action=ACT[action])
            assert ex.value.code == getattr(capi, entry["refusal"][action])
            continue
        got = scored(OrbitGrowthPlan(*case_args(c), action=ACT[action]))
        assert got == want, "%s %s: first differing seed %s" % ((entry["name"], action) + (first_diff(got, want),))


def test_both_sides_of_the_2_53_proof(hip, tmp_path):
    """one step inside: accepted and bit-exact; one step outside: PLO_E_UNSUPPORTED, and the tool announces its host loop and prints
    the winner --gpu 0 prints"""
    from plinopt_amd import OrbitGrowthPlan, OrbitPlan, capi
    by_name = {c.name: c for c, _, _ in C.bound_cases()}
    for e in GOLD["bound"]:
        c = by_name[e["name"]]
        assert c.sha256 == e["sha256"]
        if not e["refused"]:
            got = scored(OrbitGrowthPlan(*case_args(c), action=ACT[e["action"]]))
            assert got == e["out"], (e["name"], first_diff(got, e["out"]))
            continue
        with pytest.raises(capi.PloError) as ex:
            OrbitGrowthPlan(*case_args(c), action=ACT[e["action"]])
        assert ex.value.code == capi.PLO_E_UNSUPPORTED
        OrbitPlan(*case_args(c), action=ACT[e["action"]])                  # the density plan takes the same input
        outs = {}
        for g in ("1", "0"):
            d = tmp_path / (e["name"] + g)
            d.mkdir()
            src = files(c.name, str(d))
            for path, M in zip(src, (c.L, c.R, c.P)):
                open(path, "w").write(synth.sms_text(*M))
            rc, so, se = run([ORB, "-g", "--gpu", g, "--action", e["action"], "-O", "100"] + src)
            assert rc == 0, se
            outs[g] = (so, se, [open(p[:-4] + ".nnz.sms", "rb").read() if os.path.exists(p[:-4] + ".nnz.sms") else None for p in src])
        assert "host search" in outs["1"][1] and "restarts on host" in outs["1"][1]
        assert outs["1"][0] == outs["0"][0] and outs["1"][2] == outs["0"][2]


@pytest.mark.parametrize("entry", GOLD["search"], ids=lambda e: "%s-%s" % (e["name"], e["action"]))
def test_search_is_the_oracle_argmin(hip, entry):
    from plinopt_amd import OrbitGrowthPlan
    plan = OrbitGrowthPlan(*fixture_args(entry["name"]), action=ACT[entry["action"]])
    (cost, nnz, nno), seed = plan.growth_search(entry["seed0"], entry["n"])
    assert ["%016x" % G.bits(cost), nnz, nno, seed] == entry["best"]
    if entry["name"] == "2x2x2_7_Winograd":                                # signed permutations: the minimal cost is shared, the order decides
        assert entry["tied_cost"] >= 2
    # two pieces and the sharded entry on one device give the same winner
    from plinopt_amd import orbit_growth_search_multi
    a, b = plan.growth_search(0, 1000), plan.growth_search(1000, entry["n"] - 1000)
    assert min((G.bits(x[0][0]), x[0][1], x[0][2], x[1]) for x in (a, b)) == (int(entry["best"][0], 16),) + tuple(entry["best"][1:])
    got, st = orbit_growth_search_multi(*fixture_args(entry["name"]), 0, entry["n"], [0], action=ACT[entry["action"]])
    assert got == ((cost, nnz, nno), seed) and st["candidates"] == entry["n"]


@pytest.mark.parametrize("action", ["triangular", "pluq"])
@pytest.mark.parametrize("name", ["2x2x2_7_Winograd", "3x4x7_63_rational", "2x2x2_7_DPS-integral-12.0662"])
def test_cli_gpu_equals_host(hip, action, name, tmp_path):
    """(the DPS triple is outside the 2^53 proof: --gpu 1 announces the refusal and runs the host loop)"""
    out = {}
    for g in ("1", "0"):
        d = tmp_path / ("g" + g)
        d.mkdir()
        for f in files(name):
            shutil.copy(f, d)
        src = files(name, str(d))
        rc, so, se = run([ORB, "-g", "--gpu", g, "--action", action, "-O", "2000"] + src)
        assert rc == 0, se
        win = [ln for ln in se.splitlines() if "Rdcd. opt" in ln]
        out[g] = (so, win, [open(p[:-4] + ".nnz.sms", "rb").read() if os.path.exists(p[:-4] + ".nnz.sms") else None for p in src], se)
    assert out["1"][:3] == out["0"][:3]
    assert ("host search" if "DPS" in name else "restarts on GPU") in out["1"][3] and "restarts on host" in out["0"][3]
    if name == "2x2x2_7_Winograd":
        assert out["1"][1] and all(b is not None for b in out["1"][2])     # an improvement was found and written


def test_codes_of_the_refusals(hip):
    from plinopt_amd import ORBIT_ACT_HOUSEHOLDER, ORBIT_GROWTH, OrbitGrowthPlan, OrbitPlan, capi
    args = fixture_args("2x2x2_7_Winograd")
    for make in (lambda: OrbitGrowthPlan(*args, action=ORBIT_ACT_HOUSEHOLDER), lambda: OrbitGrowthPlan(*args, action=3),
                 lambda: OrbitPlan(*args, modulus=0, measure=ORBIT_GROWTH), lambda: OrbitPlan(*args, modulus=131071, measure=ORBIT_GROWTH),
                 lambda: OrbitPlan(*args, modulus=131071, measure=ORBIT_GROWTH, action=1)):
        with pytest.raises(capi.PloError) as ex:
            make()
        assert ex.value.code == capi.PLO_E_ARG
    with pytest.raises(capi.PloError) as ex:
        OrbitGrowthPlan(*args, action=ORBIT_ACT_HOUSEHOLDER)
    assert "preserves" in str(ex.value)
    plan = OrbitGrowthPlan(*args)
    for call in (lambda: plan.cost_many(seed0=0, n=4), lambda: plan.search(0, 4)):
        with pytest.raises(capi.PloError) as ex:
            call()
        assert ex.value.code == capi.PLO_E_ARG
    assert plan.info()["waves_per_wg"] in (1, 2, 4) and plan.info()["table_slots"] == (0, 0, 0)
    assert plan.growth_many(seed0=0, n=0) == []
    # a density plan is no growth plan
    import ctypes
    dens = OrbitPlan(*args)
    assert capi.lib().plo_orbit_growth_search(dens._h, 0, 4, ctypes.byref(capi.OrbitGBest()), None) == capi.PLO_E_ARG
