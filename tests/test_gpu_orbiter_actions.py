"""The PLUQ and Householder actions of the orbit search on the MI355X (plo::orbit_kernel<MOD, ACT> through
plo_orbit_plan_create_act): per-seed counts bit-exact against tests/golden/orbit_action_costs.json (the literal oracle
tests/orbit_action_oracle.py), the argmin on tie-heavy inputs, bin/orbiter --action X against --gpu 0 (winner line and written
files byte for byte), the int64 bound of each action (accepted just below, PLO_E_UNSUPPORTED just above, the tool's announced
host loop), and the default action, which is what no keyword gives."""
import json
import os
import shutil
import subprocess

import pytest

import orbit_action_cases as C
import synth
from plo_testlib import DATA, GOLDEN, ROOT, read_sms

pytestmark = pytest.mark.gpu

ORB = os.path.join(ROOT, "bin", "orbiter")
GOLD = json.load(open(os.path.join(GOLDEN, "orbit_action_costs.json")))
OLD = json.load(open(os.path.join(GOLDEN, "orbit_costs.json")))
CASES = {c.name: c for c in C.cases()}
ACT = {"triangular": 0, "pluq": 1, "householder": 2}


def run(cmd, timeout=300):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout, r.stderr


def files(name, d=DATA):
    return [os.path.join(d, "%s_%s.sms" % (name, x)) for x in "LRP"]


def fixture_args(name):
    return [synth.qcsr(*read_sms(f)) for f in files(name)]


def case_args(c):
    return [synth.qcsr(*M) for M in (c.L, c.R, c.P)]


def scored(plan, mode):
    if mode == "list":
        return [list(x) for x in plan.cost_many(C.SEEDS_LIST)]
    return [list(x) for s0, n in C.SEED_RUNS for x in plan.cost_many(seed0=s0, n=n)]


@pytest.mark.parametrize("entry", GOLD["cases"], ids=lambda e: e["name"])
def test_cost_many_bit_exact_every_entry(hip, entry):
    """fails without the feature: OrbitPlan has no keyword `action`"""
    from plinopt_amd import OrbitPlan
    args = fixture_args(entry["name"]) if entry["kind"] == "fixture" else case_args(CASES[entry["name"]])
    for key, want in sorted(entry["out"].items()):
        action, mod, ms = key.split("|")
        plan = OrbitPlan(*args, modulus=int(mod), measure=int(ms), action=ACT[action])      # nothing here is refused
        got = scored(plan, entry["mode"])
        assert got == want, "%s %s: first differing seed %s" % (entry["name"], key, next(s for s, a, b in zip(C.seeds_of(entry["mode"]), got, want) if a != b))


def test_int64_bound_of_each_action(hip, tmp_path):
    """just below the bound: accepted and bit-exact; just above: PLO_E_UNSUPPORTED, and the tool runs its host loop and says so"""
    from plinopt_amd import OrbitPlan, capi
    by_name = {c.name: c for c, _, _ in C.bound_cases()}
    for e in GOLD["bound"]:
        c = by_name[e["name"]]
        assert c.sha256 == e["sha256"]
        if not e["refused"]:
            assert scored(OrbitPlan(*case_args(c), action=ACT[e["action"]]), e["mode"]) == e["out"], e["name"]
            continue
        with pytest.raises(capi.PloError) as ex:
            OrbitPlan(*case_args(c), action=ACT[e["action"]])
        assert ex.value.code == capi.PLO_E_UNSUPPORTED
        OrbitPlan(*case_args(c))                                               # the triangular action takes the same input
        outs = {}
        for g in ("1", "0"):
            d = tmp_path / (e["name"] + g)
            d.mkdir()
            src = files(c.name, str(d))
            for path, M in zip(src, (c.L, c.R, c.P)):
                open(path, "w").write(synth.sms_text(*M))
            rc, so, se = run([ORB, "--gpu", g, "--action", e["action"], "-O", "100"] + src)
            assert rc == 0, se
            outs[g] = (so, se, [open(p[:-4] + ".nnz.sms", "rb").read() if os.path.exists(p[:-4] + ".nnz.sms") else None for p in src])
        assert "host search" in outs["1"][1] and "restarts on host" in outs["1"][1]
        assert outs["1"][0] == outs["0"][0] and outs["1"][2] == outs["0"][2]


@pytest.mark.parametrize("entry", GOLD["tie"], ids=lambda e: "%s-%s" % (e["name"], e["action"]))
def test_search_on_ties_is_the_golden_argmin(hip, entry):
    from plinopt_amd import OrbitPlan
    c = {(c.name, C.ACTION_NAMES[a]): c for c, a in C.tie_cases()}[(entry["name"], entry["action"])]
    assert c.sha256 == entry["sha256"]
    o, s0, n = entry["out"], entry["seed0"], entry["n"]
    want = min((o[3 * j], o[3 * j + 1], o[3 * j + 2], s0 + j) for j in range(n))
    assert sum(1 for j in range(n) if tuple(o[3 * j:3 * j + 3]) == want[:3]) > 1          # the minimum is tied
    plan = OrbitPlan(*case_args(c), modulus=c.modulus, measure=c.measure, action=ACT[entry["action"]])
    (cost, nnz, nno), seed = plan.search(s0, n)
    assert (cost, nnz, nno, seed) == want


@pytest.mark.parametrize("action", ["pluq", "householder"])
@pytest.mark.parametrize("name,args", [("2x2x2_7_Winograd", ["-O", "2000"]), ("4x4x4_49_156", ["-c", "-O", "2000"]),
                                       ("2x2x2_7_Winograd", ["-m", "131071", "-O", "2000"]), ("4x4x4_49_156", ["-m", "131071", "-O", "2000"])])
def test_cli_gpu_equals_host(hip, action, name, args, tmp_path):
    out = {}
    for g in ("1", "0"):
        d = tmp_path / ("g" + g)
        d.mkdir()
        for f in files(name):
            shutil.copy(f, d)
        src = files(name, str(d))
        rc, so, se = run([ORB, "--gpu", g, "--action", action] + args + src)
        assert rc == 0, se
        out[g] = (so, se, [open(p[:-4] + ".nnz.sms", "rb").read() if os.path.exists(p[:-4] + ".nnz.sms") else None for p in src])
    assert out["1"][0] == out["0"][0] and out["1"][2] == out["0"][2]
    assert "restarts on GPU" in out["1"][1] and "restarts on host" in out["0"][1]


@pytest.mark.parametrize("action", ["pluq", "householder"])
def test_search_multi_shards_equal_one_device(hip, action):
    from plinopt_amd import OrbitPlan, orbit_search_multi
    args = fixture_args("3x3x3_23_58")
    one = OrbitPlan(*args, action=ACT[action]).search(1000, 3001)
    for nd in (1, 3):
        got, st = orbit_search_multi(*args, 0, 0, 1000, 3001, [0] * nd, action=ACT[action])
        assert got == one and st["candidates"] == 3001


def test_default_action_is_the_triangular_one(hip):
    from plinopt_amd import ORBIT_ACT_TRIANGULAR, OrbitPlan, capi
    L = OLD["long"]
    args = fixture_args(L["name"])
    want = [tuple(L["out3"][3 * j:3 * j + 3]) for j in range(L["n"])]
    assert OrbitPlan(*args, action=ORBIT_ACT_TRIANGULAR).cost_many(seed0=L["seed0"], n=L["n"]) == want
    assert OrbitPlan(*args).cost_many(seed0=L["seed0"], n=L["n"]) == want
    with pytest.raises(capi.PloError) as ex:
        OrbitPlan(*args, action=3)
    assert ex.value.code == capi.PLO_E_ARG
