"""The exact CSE restart search over Q on the GPU (plo_cse_plan_create_q; bin/optimizer --gpu-q) against the goldens of the Python
restatement over exact fractions (tests/golden/cse_q_costs.json): per-seed costs, the searches of all three cost modes, the
refusals, the prime knob and the tool.  A case that must run and that the device refuses fails: nothing is skipped."""
import os
import random
import re
import subprocess

import pytest

import cse_q_cases as Q
from plinopt_amd import CSEPlanQ, capi, cmp_op_count_key, cse_q_universe
from plo_testlib import DATA, ROOT
from fractions import Fraction as F

pytestmark = pytest.mark.gpu
OPT = os.path.join(ROOT, "bin", "optimizer")
CHK = os.path.join(ROOT, "bin", "SLPchecker")
CASES = Q.cases()
RUNNING = [c for c in CASES if not c.refused]
GOLD = Q.goldens()
MODES = (capi.COST_SUM_THEN_ADD, capi.COST_ADD_THEN_MUL, capi.COST_SUM)


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "plinopt_amd", "csrc", "host")])


@pytest.fixture(autouse=True)
def _no_knob(monkeypatch):
    monkeypatch.delenv("PLO_CSE_Q_PRIME", raising=False)


def check_against_goldens(plan, c):
    gold = GOLD[c.name]
    n = len(gold)
    a, mu = plan.cost_many(seed0=0, n=n)
    got = list(zip(a, mu))
    bad = [s for s in range(n) if got[s] != gold[s]]
    assert not bad, (c.name, "seeds", bad[:8], [(got[s], gold[s]) for s in bad[:4]])
    seeds = list(range(n))
    random.Random(7).shuffle(seeds)
    a, mu = plan.cost_many(seeds=seeds)
    assert list(zip(a, mu)) == [gold[s] for s in seeds], c.name
    for mode in MODES:
        best = min(range(n), key=lambda s: (cmp_op_count_key(gold[s][0], gold[s][1], mode), s))
        assert plan.search(0, n, mode) == (gold[best][0], gold[best][1], best), (c.name, mode)


@pytest.mark.parametrize("c", RUNNING, ids=lambda c: c.name)
def test_costs_and_searches_equal_the_goldens(hip, c):
    plan = CSEPlanQ(*Q.csr_q(c))
    try:
        assert not plan.is_hbm
        check_against_goldens(plan, c)
    finally:
        plan.close()


def test_enumeration_is_refused_on_a_plan_over_q(hip):
    c = next(c for c in CASES if c.name == "tie_order")
    plan = CSEPlanQ(*Q.csr_q(c))
    with pytest.raises(capi.PloError) as e:
        plan.enum_cost_many(0, 4)
    assert e.value.code == capi.PLO_E_UNSUPPORTED
    with pytest.raises(capi.PloError) as e:
        plan.enum_search(0, 4)
    assert e.value.code == capi.PLO_E_UNSUPPORTED
    plan.close()


@pytest.mark.parametrize("c", [c for c in CASES if c.refused], ids=lambda c: c.name)
def test_refused_cases(hip, c):
    with pytest.raises(capi.PloError) as e:
        CSEPlanQ(*Q.csr_q(c))
    assert e.value.code == c.refused and c.why in str(e.value)


def test_prime_knob_7_refuses(hip, monkeypatch):
    monkeypatch.setenv("PLO_CSE_Q_PRIME", "7")
    with pytest.raises(capi.PloError) as e:
        CSEPlanQ(*Q.csr_q(next(c for c in CASES if c.name == "tie_order")))
    assert e.value.code == capi.PLO_E_UNSUPPORTED and "no prime among" in str(e.value)


def test_colliding_prime_steps_to_the_next_and_still_matches(hip, monkeypatch):
    c = next(c for c in CASES if c.name == "collide")
    U = [F(n, d) for n, d in cse_q_universe(*Q.csr_q(c))[2]]
    bad = Q.colliding_prime(U)
    assert bad is not None and not Q.separates(U, bad)
    monkeypatch.setenv("PLO_CSE_Q_PRIME", str(bad))
    plan = CSEPlanQ(*Q.csr_q(c))
    try:
        assert plan.prime == Q.prime_below(bad)
        check_against_goldens(plan, c)
    finally:
        plan.close()
    # and the step the plan takes by itself: 2147483629 divides a numerator of prime_step
    monkeypatch.delenv("PLO_CSE_Q_PRIME")
    c = next(c for c in CASES if c.name == "prime_step")
    plan = CSEPlanQ(*Q.csr_q(c))
    assert plan.prime == Q.prime_below(Q.PRIME0)
    plan.close()


def run(cmd, stdin=None):
    r = subprocess.run(cmd, input=stdin, capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("name", ["2x2x2_7_DPS-accurate_L", "4x4x4_48_rational_L", "3x4x7_63_rational_R"])
def test_optimizer_gpu_q_prints_the_host_program(name):
    path = os.path.join(DATA, name + ".sms")
    rc, out, err = run([OPT, "--gpu-q", "--only", "D", "-O", "2000", path])
    assert rc == 0 and "# GPU (over Q): 2000 candidates" in err and "refused" not in err and "ERROR" not in err, err
    rc0, out0, err0 = run([OPT, "--gpu", "0", "--only", "D", "-O", "2000", path])
    assert rc0 == 0 and "# host search" in err0, err0
    assert out == out0 and out
    found = re.search(r"# Found D: (\d+\|\d+) instead of .*\[seed (\d+)\]", err), re.search(r"# Found D: (\d+\|\d+) instead of .*\[seed (\d+)\]", err0)
    assert found[0] and found[1] and found[0].groups() == found[1].groups()
    rc, _, err2 = run([CHK, "-M", path], stdin=out)
    assert rc == 0 and "SUCCESS" in err2, err2


def test_optimizer_gpu_q_says_a_refusal_and_searches_on_the_host(tmp_path):
    c = next(c for c in CASES if c.name == "values65")
    path = str(tmp_path / "values65.sms")
    with open(path, "w") as f:
        f.write(Q.sms_text(c))
    rc, out, err = run([OPT, "--gpu-q", "--only", "D", "-O", "200", path])
    assert rc == 0 and "# -D on the GPU refused (65 distinct values" in err and "): host search" in err and "# host search: 200 candidates" in err, err
    rc0, out0, _ = run([OPT, "--gpu", "0", "--only", "D", "-O", "200", path])
    assert rc0 == 0 and out == out0 and out
