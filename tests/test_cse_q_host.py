"""The exact CSE restart search over Q, host side (no device): the Python restatement tests/cse_q_oracle.py is held to the C oracle
modulo two primes and to bin/optimizer --replay over Q; the goldens tests/golden/cse_q_costs.json to the restatement; the universe U
of plo_cse_q_universe to what the restatement compares; the refusals of plo_cse_plan_create_q to their codes and texts, which come
before any device call."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction as F

import pytest

import cse_q_cases as Q
import cse_q_oracle as O
from plinopt_amd import capi, cse_q_universe
from plinopt_amd.search import _qcsr
from plo_testlib import ROOT, OracleMatrix, to_csr_mod

OPT = os.path.join(ROOT, "bin", "optimizer")
CASES = Q.cases()
RUNNING = [c for c in CASES if not c.refused]
GOLD = Q.goldens()
PRIMES = (2147483629, 131071)
FIRST = 4


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "plinopt_amd", "csrc", "host")])


def q_costs(c, seeds, F_=None):
    Fq = F_ or O.QQ()
    rows = O.field_rows(Fq, c.m, c.ent)
    return [O.Optimizer(Fq, rows, c.n, s).run() for s in seeds]


def test_goldens_cover_the_running_cases():
    assert sorted(GOLD) == sorted(c.name for c in RUNNING)
    for c in RUNNING:
        assert len(GOLD[c.name]) == c.nseeds, c.name
    by = {c.name: c for c in CASES}
    assert by["4x4x4_48_rational_L"].nseeds == 150 and by["tie_order"].nseeds == 256 and by["4o4o8_Toom5_P"].nseeds == 64


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_restatement_over_zp_equals_the_c_oracle(c):
    """validates the restatement: its Z_p instance against oracle/plo_oracle.c on the image of every case modulo two primes"""
    for p in PRIMES:
        rp, col, val = to_csr_mod(c.m, c.n, c.ent, p)
        a, mu = OracleMatrix(c.m, c.n, rp, col, val, p).cost_many(seed0=0, nseeds=FIRST)
        assert q_costs(c, range(FIRST), O.Zp(p)) == list(zip(a, mu)), (c.name, p)


@pytest.mark.parametrize("c", RUNNING, ids=lambda c: c.name)
def test_goldens_equal_the_restatement_over_q(c):
    assert q_costs(c, range(FIRST)) == GOLD[c.name][:FIRST]


@pytest.mark.parametrize("c", [c for c in RUNNING if c.fixture], ids=lambda c: c.name)
def test_goldens_equal_the_host_replay_over_q(tools, c):
    for s in range(16):
        r = subprocess.run([OPT, "--replay", "--seed", str(s), c.fixture], capture_output=True, text=True, timeout=120)
        m = re.search(r"# (\d+)\tadditions\n# (\d+)\tmultiplications", r.stderr)
        assert r.returncode == 0 and m, r.stderr
        assert (int(m.group(1)), int(m.group(2))) == GOLD[c.name][s], (c.name, s)


def test_a_residue_ordered_search_is_another_search():
    """4x4x4_48_rational_L: the costs over Q differ from the costs modulo 2147483629 on at least 10 of the seeds 0..149 (17 today)"""
    c = next(c for c in CASES if c.name == "4x4x4_48_rational_L")
    a, mu = OracleMatrix.from_sms(c.fixture, PRIMES[0]).cost_many(seed0=0, nseeds=150, nthreads=4)
    differ = [s for s in range(150) if GOLD[c.name][s] != (a[s], mu[s])]
    print("seeds that differ:", len(differ), differ)
    assert len(differ) >= 10


def test_tie_order_case_differs_too():
    """the 4 x 5 case: a column pair tied at two ratios that Q and the residues order differently, and costs that differ -- by both
    oracles, the restatement modulo p and the C oracle"""
    c = next(c for c in CASES if c.name == "tie_order")
    p, zp = PRIMES[0], O.Zp(PRIMES[0])
    o = O.Optimizer(O.QQ(), O.field_rows(O.QQ(), c.m, c.ent), c.n, 0)
    pm = {}
    for row in o.M:
        for t in o.listpairs(row):
            pm[t] = pm.get(t, 0) + 1
    top = sorted(t for t, f in pm.items() if f == max(pm.values()))
    assert max(pm.values()) >= 2
    assert any(x[:2] == y[:2] and zp.conv(x[2]) > zp.conv(y[2]) for x, y in zip(top, top[1:])), top
    seeds = range(32)
    modp = q_costs(c, seeds, zp)
    rp, col, val = to_csr_mod(c.m, c.n, c.ent, p)
    a, mu = OracleMatrix(c.m, c.n, rp, col, val, p).cost_many(seed0=0, nseeds=32)
    assert modp == list(zip(a, mu))
    differ = [s for s in seeds if GOLD[c.name][s] != modp[s]]
    print("seeds that differ:", len(differ))
    assert len(differ) >= 4


def test_triangle_cases_fire():
    for name in ("triangle", "triangle_neg"):
        c = next(c for c in CASES if c.name == name)
        o = O.Optimizer(O.QQ(), O.field_rows(O.QQ(), c.m, c.ent), c.n, 0)
        o.run()
        assert o.triangles >= 1, name


@pytest.mark.parametrize("c", RUNNING, ids=lambda c: c.name)
def test_universe_holds_what_a_candidate_compares(c):
    prime, nv, U = cse_q_universe(*Q.csr_q(c))
    U = [F(n, d) for n, d in U]
    assert nv == len(set(c.ent.values())) <= 64
    assert all(x < y for x, y in zip(U, U[1:])), "U ascending"
    assert [-u for u in reversed(U)] == U and F(1) in U
    assert Q.is_prime(prime) and prime < 2 ** 31 and Q.separates(U, prime)
    Fq = O.QQ()
    Fq.seen = set()
    q_costs(c, range(FIRST), Fq)
    assert Fq.seen <= set(U), sorted(Fq.seen - set(U))[:5]


def test_counts_of_the_value_limits():
    by = {c.name: c for c in CASES}
    assert len(set(by["values64"].ent.values())) == 64 and len(set(by["values65"].ent.values())) == 65
    assert cse_q_universe(*Q.csr_q(by["values64"]))[1] == 64


def _create(c_or_csr, flags=0):
    A, keep = _qcsr(*(Q.csr_q(c_or_csr) if hasattr(c_or_csr, "ent") else c_or_csr))
    h = ctypes.c_void_p()
    rc = capi.lib().plo_cse_plan_create_q(ctypes.byref(A), flags, ctypes.byref(h))
    msg = capi.lib().plo_last_error().decode()
    if rc == capi.PLO_OK:
        capi.lib().plo_cse_plan_destroy(h)
    return rc, msg


def _universe_rc(c, cap=0):
    A, keep = _qcsr(*Q.csr_q(c))
    out = [ctypes.c_uint32() for _ in range(3)]
    num, den = (ctypes.c_int64 * max(cap, 1))(), (ctypes.c_int64 * max(cap, 1))()
    rc = capi.lib().plo_cse_q_universe(ctypes.byref(A), *[ctypes.byref(x) for x in out], num, den, cap)
    return rc, [x.value for x in out], capi.lib().plo_last_error().decode()


def test_refusals_and_their_texts_come_before_the_device(monkeypatch):
    monkeypatch.delenv("PLO_CSE_Q_PRIME", raising=False)
    by = {c.name: c for c in CASES}
    for c in CASES:
        if c.refused:
            rc, msg = _create(c)
            assert rc == c.refused == capi.PLO_E_UNSUPPORTED and c.why in msg, (c.name, rc, msg)
            assert _universe_rc(c)[0] == capi.PLO_E_UNSUPPORTED
    assert _universe_rc(by["values65"])[1][1] == 65
    # the HBM-resident family: asked for, or needed (a row of 65 entries, 70 rows with a coefficient 2)
    rc, msg = _create(by["tie_order"], capi.PLAN_HBM)
    assert rc == capi.PLO_E_UNSUPPORTED and "HBM" in msg
    rc, msg = _create((1, 65, [0, 65], list(range(65)), [1] * 64 + [-1], None))
    assert rc == capi.PLO_E_UNSUPPORTED and "HBM-resident" in msg and "64 entries" in msg, msg
    rc, msg = _create((70, 2, list(range(0, 141, 2)), [0, 1] * 70, [1, 2] * 70, None))
    assert rc == capi.PLO_E_UNSUPPORTED and "HBM-resident" in msg, msg
    # arguments
    h = ctypes.c_void_p()
    assert capi.lib().plo_cse_plan_create_q(None, 0, ctypes.byref(h)) == capi.PLO_E_ARG
    assert _create(by["tie_order"], 2)[0] == capi.PLO_E_ARG
    assert _create((1, 2, [0, 2], [1, 0], [1, 1], None))[0] == capi.PLO_E_ARG             # columns not increasing
    assert _create((1, 2, [0, 2], [0, 1], [1, 0], None))[0] == capi.PLO_E_ARG             # a zero entry
    assert _create((1, 2, [0, 2], [0, 1], [1, 1], [1, -3]))[0] == capi.PLO_E_ARG          # a negative denominator
    # the universe: too small a capacity reports the counts
    rc, out, msg = _universe_rc(by["tie_order"], cap=3)
    assert rc == capi.PLO_E_CAPACITY and out[0] == PRIMES[0] and out[1] == len(set(by["tie_order"].ent.values())) == 7 and out[2] == 26, (rc, out, msg)
    big = 3037000507                                                                      # big^2 passes 2^63, big^4 stays below 2^127
    wide = Q.SimpleNamespace(m=1, n=2, ent={(0, 0): F(big), (0, 1): F(1, big)})
    rc, out, msg = _universe_rc(wide, cap=64)
    assert rc == capi.PLO_E_CAPACITY and "64 bits" in msg and out[1:] == [2, 10], (rc, out, msg)


def test_prime_knob(monkeypatch):
    by = {c.name: c for c in CASES}
    monkeypatch.setenv("PLO_CSE_Q_PRIME", "7")
    rc, msg = _create(by["tie_order"])
    assert rc == capi.PLO_E_UNSUPPORTED and "no prime among the first 8 from 7 down (7, 5, 3)" in msg, msg
    # the step to the next prime: by itself (2147483629 divides a numerator) and forced
    monkeypatch.delenv("PLO_CSE_Q_PRIME")
    assert cse_q_universe(*Q.csr_q(by["prime_step"]))[0] == Q.prime_below(PRIMES[0]) == 2147483587
    prime, _, U = cse_q_universe(*Q.csr_q(by["collide"]))
    assert prime == PRIMES[0]
    bad = Q.colliding_prime([F(n, d) for n, d in U])
    assert bad == 2 ** 30 + 3
    monkeypatch.setenv("PLO_CSE_Q_PRIME", str(bad))
    assert cse_q_universe(*Q.csr_q(by["collide"]))[0] == Q.prime_below(bad)
