"""The CSE measure of the orbit search on the MI355X (plo::orbit_cse_kernel through plo_orbit_plan_create_cse; bin/orbiter -z):
per-seed (cost, nnz, nno) bit-exact against the literal oracle tests/orbit_cse_oracle.py on fixture, synthetic and edge triples,
announced refusals, the repeat-with-larger-tables path, the argmin of the searches and bin/orbiter --gpu 1 against --gpu 0.
Every parity test here fails without the feature (the parent has no plo_orbit_plan_create_cse; OrbitPlan has no `sub`)."""
import functools
import os
import shutil
import subprocess
from fractions import Fraction as F

import pytest

import orbit_cse_oracle as Z
import orbit_oracle as O
import synth
from plo_testlib import DATA, ROOT, read_sms

pytestmark = pytest.mark.gpu

ORB = os.path.join(ROOT, "bin", "orbiter")
BASE = O.BASE_SEED


def files(name, d=DATA):
    return [os.path.join(d, "%s_%s.sms" % (name, x)) for x in "LRP"]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(qcsr arguments, dense matrices, (m, k, n))"""
    mats, mkn = O.load(os.path.join(DATA, name))
    return [synth.qcsr(*read_sms(f)) for f in files(name)], mats, mkn


def triple(L, R, P):
    """the same from three (m, n, entries) matrices"""
    mats = [O.dense(*M) for M in (L, R, P)]
    mats = [M if O.small_ints(M) is None else O.small_ints(M) for M in mats]
    return [synth.qcsr(*M) for M in (L, R, P)], mats, O.shape(*[(M[0], M[1]) for M in (L, R, P)])


def naive_algorithm(m, k, n):
    """row (a, b, c): e_{ak+b}, e_{bn+c}; column e_{an+c}"""
    L, R, P = {}, {}, {}
    for a in range(m):
        for b in range(k):
            for c in range(n):
                t = (a * k + b) * n + c
                L[(t, a * k + b)] = F(1); R[(t, b * n + c)] = F(1); P[(a * n + c, t)] = F(1)
    r = m * k * n
    return (r, m * k, L), (r, k * n, R), (m * n, r, P)


def plan_of(args, p, sub, cse_seed0=0, action=0):
    from plinopt_amd import ORBIT_CSE, OrbitPlan
    return OrbitPlan(*args, modulus=p, measure=ORBIT_CSE, action=action, sub=sub, cse_seed0=cse_seed0)


def parity(tr, seeds, p, sub, cse_seed0=0, action=0, may_refuse=False):
    """cost_many of the device == the oracle; with may_refuse a PLO_E_CAPACITY refusal (with its reason) is the other outcome.
    Returns the plan, or None when refused."""
    from plinopt_amd import capi
    args, mats, mkn = tr
    try:
        plan = plan_of(args, p, sub, cse_seed0, action)
    except capi.PloError as e:
        assert may_refuse and e.code == capi.PLO_E_CAPACITY and "CSE measure" in str(e), e
        return None
    got = plan.cost_many(seeds)
    want, _ = Z.costs(mats, mkn, seeds, p, sub, cse_seed0, action)
    assert got == want, next((s, a, b) for s, a, b in zip(seeds, got, want) if a != b)
    return plan


@pytest.mark.parametrize("p", [131071, 3, 2147483629])
@pytest.mark.parametrize("sub", [1, 3])
def test_winograd_256_seeds_and_the_base(hip, p, sub):
    assert parity(fixture("2x2x2_7_Winograd"), [BASE] + list(range(256)), p, sub)


@pytest.mark.parametrize("action", [0, 1, 2], ids=["triangular", "pluq", "householder"])
def test_strassen_every_action(hip, action):
    assert parity(fixture("2x2x2_7_Strassen"), [BASE] + list(range(64)), 131071, 2, 0, action)


@pytest.mark.parametrize("cse_seed0", [0, 7])
def test_3x3x3_23_58(hip, cse_seed0):
    plan = parity(fixture("3x3x3_23_58"), [BASE] + list(range(64)), 131071, 2, cse_seed0)
    assert plan and plan.info()["relaunches"] == 0


def test_3x4x7_63_one_below_the_row_limit(hip):
    """r = 63 and a 21 x 63 P part, one below the row limit: parity, or the announced refusal.  On the MI355X it is refused with
    PLO_E_CAPACITY: the image of a candidate does not fit LDS with one wave."""
    plan = parity(fixture("3x4x7_63_rational"), [BASE, 0, 1, 2], 131071, 2, may_refuse=True)
    print("3x4x7_63_rational:", "refused" if plan is None else plan.info())


def test_modular_synthetic_cases_match_or_are_refused(hip):
    def prime(q):
        return q > 2 and all(q % d for d in range(2, int(q ** 0.5) + 1))
    cases = [c for c in synth.orbit_cases() if c.modulus and c.refusal is None and prime(c.modulus)]
    assert len(cases) >= 8
    ran = 0
    for c in cases:
        plan = parity(triple(c.L, c.R, c.P), [BASE, 0, 1, 2, 5, 1 << 40], c.modulus, 2, may_refuse=True)
        m, k, n = c.mkn
        assert (plan is None) == (max(m * k, k * n, m * n, c.r) > 64), c.name      # the only reason these shapes can be refused for
        ran += plan is not None
    assert ran >= 6


@pytest.mark.parametrize("mkn", [(1, 1, 1), (1, 1, 3), (3, 1, 1), (2, 2, 2), (8, 8, 1)], ids=lambda s: "%dx%dx%d" % s)
def test_naive_algorithms_at_the_edges(hip, mkn):
    """r = 1 without any pair, rows of one entry, r = 8, and r = 64 with rows of up to 64 entries.  The last one is refused on the
    MI355X, with sub = 1 too: Lj is 64 x 64 with up to 4096 entries, and its image with the pair table does not fit LDS with one wave
    (tests/test_gpu_orbiter_cse_edges.py runs 64 columns and 64 rows on images that fit)."""
    from plinopt_amd import capi
    tr = triple(*naive_algorithm(*mkn))
    if mkn == (8, 8, 1):
        with pytest.raises(capi.PloError) as e:
            plan_of(tr[0], 131071, 2)
        assert e.value.code == capi.PLO_E_CAPACITY and "CSE measure: the image of a candidate does not fit LDS with one wave" in str(e.value), e.value
        return
    plan = parity(tr, [BASE] + list(range(32)), 131071, 2)
    print(mkn, plan.info())


def test_empty_row_of_L_and_empty_column_of_P(hip):
    L, R, P = naive_algorithm(2, 2, 2)
    L = (9, 4, dict(L[2])); R = (9, 4, dict(R[2])); P = (4, 9, dict(P[2]))
    R[2][(8, 1)] = F(1); R[2][(8, 2)] = F(-2)                                 # row 8: nothing in L, two entries in R, nothing in P
    assert parity(triple(L, R, P), [BASE] + list(range(32)), 131071, 2)


def test_full_table_repeats_the_launch_with_more_slots(hip, monkeypatch):
    tr = fixture("3x3x3_23_58")
    seeds = [BASE] + list(range(16))
    want = plan_of(tr[0], 131071, 2).cost_many(seeds)
    monkeypatch.setenv("PLO_ORBIT_CSE_CAP", "64")
    plan = plan_of(tr[0], 131071, 2)
    assert plan.info()["table_slots"] == (64, 64, 64)
    assert plan.cost_many(seeds) == want
    info = plan.info()
    assert info["relaunches"] >= 1 and min(info["table_slots"]) >= 128
    assert want == Z.costs(tr[1], tr[2], seeds, 131071, 2, 0)[0]


@functools.lru_cache(maxsize=None)
def winograd_2000():
    _, mats, mkn = fixture("2x2x2_7_Winograd")
    return Z.costs(mats, mkn, list(range(2000)), 131071, 2, 0)


def test_search_is_the_oracles_lexicographic_minimum(hip):
    per, best = winograd_2000()
    assert sum(1 for c in per if c == best[:3]) > 1                            # the minimum is tied: the seed decides
    plan = plan_of(fixture("2x2x2_7_Winograd")[0], 131071, 2)
    assert plan.search(0, 2000) == (best[:3], best[3])
    a, b = plan.search(0, 1200), plan.search(1200, 800)                        # two pieces
    assert min(a, b) == (best[:3], best[3])
    assert a == min((c, s) for s, c in enumerate(per[:1200]))
    assert plan.last_stats["candidates"] == 800


def test_search_multi_cse_with_one_device(hip):
    from plinopt_amd import ORBIT_CSE, orbit_search_multi
    per, best = winograd_2000()
    got, st = orbit_search_multi(*fixture("2x2x2_7_Winograd")[0], 131071, ORBIT_CSE, 0, 2000, [0], sub=2)
    assert got == (best[:3], best[3]) and st["candidates"] == 2000


def test_cli_gpu_equals_host(hip, tmp_path):
    out = {}
    for g in ("1", "0"):
        d = tmp_path / ("g" + g)
        d.mkdir()
        for f in files("2x2x2_7_Strassen"):
            shutil.copy(f, d)
        src = files("2x2x2_7_Strassen", str(d))
        r = subprocess.run([ORB, "--gpu", g, "-q", "131071", "-z", "-O", "200"] + src, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out[g] = (r.stdout, r.stderr, [open(p[:-4] + ".nnz.sms", "rb").read() if os.path.exists(p[:-4] + ".nnz.sms") else None for p in src])
    assert out["1"][0] == out["0"][0] and out["1"][2] == out["0"][2] and out["1"][2][0] is not None
    assert "restarts on GPU" in out["1"][1] and "restarts on host" in out["0"][1]
    assert "%d Optimizer runs" % (200 * 3 * 12) in out["1"][1]
