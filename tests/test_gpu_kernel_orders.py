"""`bin/optimizer -N` by order index on the device (plo::kmethod_orders_kernel through `plo_kernel_search_orders`): candidate
by candidate against the oracle's prescribed-order decomposition (oracle/plo_oracle.c `plo_oracle_kernel_order`), the
minimum under (cost key, candidate index), ranges that compose, launches that chunk, the refusals and the tool.  (The k-th
permutation that kernel_orders_lib restates is checked against itertools in test_kernel_orders_host.py.)"""
import math
import os
import re
import subprocess

import pytest

from kernel_orders_lib import P, csr_args, distinct, fixture, kth_permutation, oracle_best, oracle_range, synthetic12
from plo_testlib import DATA, ROOT

pytestmark = pytest.mark.gpu
OPT = os.path.join(ROOT, "bin", "optimizer")
CHK = os.path.join(ROOT, "bin", "SLPchecker")
F = math.factorial
S243_L = os.path.join(DATA, "4o4o4_S243_10-43_L.sms")
CLI_RANGE = (1814144, 2000)          # 5 * 9! - 256: the range of the tool's bounded run
N_PAT = r"# Found N: (\d+)\|(\d+) instead of \d+\|\d+\t\[order (\d+), seed (\d+)\] \((\d+) of (\d+) row orders from (\d+), (\d+) restarts each, (GPU kernel [0-9.e+-]+ ms|host)\)"


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "plinopt_amd", "csrc", "host")])


def run(cmd, stdin=None, env=None):
    r = subprocess.run(cmd, input=stdin, capture_output=True, text=True, timeout=600, env=env)
    return r.returncode, r.stdout, r.stderr


def check_range(M, seed0, first, count, sub, cost_modes=(0,), min_distinct=0):
    """every candidate of the range and the best of each cost mode equal the oracle's"""
    from plinopt_amd import kernel_search_orders
    exp = oracle_range(M, seed0, first, count, sub)
    assert distinct(exp) >= min_distinct, distinct(exp)
    for mode in cost_modes:
        adds, muls, info, best, st = kernel_search_orders(csr_args(M), P, seed0, first, count, sub, cost_mode=mode)
        got = [(a, mu) + i for a, mu, i in zip(adds, muls, info)]
        bad = [k for k in range(len(exp)) if got[k] != exp[k]]
        assert not bad, (len(bad), bad[:5], [(got[k], exp[k]) for k in bad[:5]])
        assert best == oracle_best(exp, seed0, first, sub, mode), mode
        assert st["candidates"] == count * sub and st["launches"] >= 2          # the sizing launch + the search
    return exp


def test_every_order_of_seven_rows(hip):
    """(a) all 5040 orders of 2x2x2_7_Winograd_L, two restarts each; the best under all three cost modes"""
    check_range(fixture("2x2x2_7_Winograd_L"), 11, 0, 5040, 2, cost_modes=(0, 1, 2))


@pytest.mark.parametrize("name,m", [("4o4o4_S243_10-43_L", 10), ("4o4o4_F243-11-44_R", 11)])
@pytest.mark.parametrize("where", ["start", "carry", "end", "end509"])
def test_ranges_of_ten_and_eleven_rows(hip, name, m, where):
    """(b) ranges of 512 orders, sub = 2: the first orders, a carry in the leading factoradic digit, the last orders; and the last 509
    (no multiple of the waves of a workgroup)"""
    M = fixture(name)
    assert M.m == m
    first, count = {"start": (0, 512), "carry": (5 * F(m - 1) - 256, 512), "end": (F(m) - 512, 512), "end509": (F(m) - 509, 509)}[where]
    check_range(M, 11, first, count, 2, min_distinct=30)


@pytest.mark.parametrize("kind", ["mixed", "unit"])
@pytest.mark.parametrize("first", [F(12) - 300, 7 * F(11) - 100])
def test_ranges_of_twelve_rows(hip, kind, first):
    """(c) 12 rows (an empty row and two equal rows in "mixed"; +-1 entries only in "unit"), sub = 3, seed0 beyond 2^40: the candidate
    index and both seeds are 64-bit"""
    M = synthetic12(kind)
    if kind == "mixed":
        d = M.dense()
        row = lambda i: {j: v for (r, j), v in d.items() if r == i}
        assert row(4) == {} and row(9) == row(2) != {} and set(M.val) == {1, P - 1, 2, 3}
    else:
        assert all(x in (1, P - 1) for x in M.val)
    check_range(M, 2 ** 40 + 5, first, 300, 3, min_distinct=30)


def test_ranges_compose_and_calls_chunk(hip, monkeypatch):
    """(d) best of [a, a+600) = the better of its halves, the earlier one on a tie; the same call in launches of 250 candidates
    (PLO_KORD_CHUNK) returns the same best and every candidate, and its statistics are sums over the launches"""
    from plinopt_amd import kernel_search_orders
    M, seed0, a, sub = fixture("4o4o4_S243_10-43_L"), 11, 5 * F(9) - 256, 2
    key = lambda b: (b[0] + b[1], b[0])
    whole = kernel_search_orders(csr_args(M), P, seed0, a, 600, sub)
    lo = kernel_search_orders(csr_args(M), P, seed0, a, 300, sub, want_costs=False)
    hi = kernel_search_orders(csr_args(M), P, seed0, a + 300, 300, sub, want_costs=False)
    assert whole[3] == (lo[3] if key(lo[3]) <= key(hi[3]) else hi[3])
    assert whole[3] == oracle_best(oracle_range(M, seed0, a, 600, sub), seed0, a, sub)
    monkeypatch.setenv("PLO_KORD_CHUNK", "250")
    parts = kernel_search_orders(csr_args(M), P, seed0, a, 600, sub)
    assert parts[:4] == whole[:4]
    assert parts[4]["candidates"] == whole[4]["candidates"] == 1200
    assert whole[4]["launches"] >= 2 and parts[4]["launches"] >= 1 + 5          # 1200 candidates in launches of 250, behind the sizing launch
    assert parts[4]["kernel_ms"] > 0


def test_a_launch_that_overflows_is_repeated_and_the_walk_goes_on(hip, monkeypatch):
    """Dep's arrays come from a sample of the range; a launch that meets a larger Dep reports it, is repeated with the hard bounds, and
    the launches after it keep them (here the first size is forced 8 times too small, the call is 5 launches): the oracle's results"""
    monkeypatch.setenv("PLO_KMETHOD_ENT_DIV", "8")
    monkeypatch.setenv("PLO_KORD_CHUNK", "250")
    from plinopt_amd import kernel_search_orders
    M, seed0, a, sub = fixture("4o4o4_F243-11-44_R"), 11, 5 * F(10) - 256, 2
    adds, muls, info, best, st = kernel_search_orders(csr_args(M), P, seed0, a, 512, sub)
    exp = oracle_range(M, seed0, a, 512, sub)
    assert tuple((x, y) + i for x, y, i in zip(adds, muls, info)) == exp
    assert best == oracle_best(exp, seed0, a, sub)
    assert st["launches"] >= 1 + 1 + 5 and st["candidates"] == 1024          # sizing, the undersized launch, 5 launches of at most 250


def test_refusals(hip):
    """(e)"""
    from plinopt_amd import capi, kernel_search_orders
    ident = (10, 10, list(range(11)), list(range(10)), [1] * 10)
    rows13 = (13, 2, list(range(14)), [0] * 13, [1] * 13)
    M = fixture("4o4o4_S243_10-43_L")
    for args, code in ((( ident, P, 0, 0, 10), capi.PLO_E_UNSUPPORTED),
                       ((rows13, P, 0, 0, 10), capi.PLO_E_ARG),
                       ((csr_args(M), P, 0, F(10) - 9, 10), capi.PLO_E_ARG),          # first + count = 10! + 1
                       ((csr_args(M), P, 0, 0, 10, 0), capi.PLO_E_ARG)):             # sub = 0
        with pytest.raises(capi.PloError) as e:
            kernel_search_orders(*args)
        assert e.value.code == code, (args[1:], e.value)
    assert kernel_search_orders(csr_args(M), P, 0, F(10) - 10, 10)[4]["candidates"] == 10      # first + count = 10!


def found_n(err):
    g = re.search(N_PAT, err)
    assert g, err
    return tuple(int(x) for x in g.groups()[:8]), g.group(9)


def test_tool_on_a_range_gpu_equals_host_equals_oracle():
    """(f) --orders on the 10-row fixture: device and host print the same program and the same winner, which is the oracle's argmin;
    the program checks"""
    first, count = CLI_RANGE
    cmd = [OPT, "-q", str(P), "--only", "N", "--orders", "%d:%d" % CLI_RANGE, "--seed", "11", S243_L]
    rc, out, err = run(cmd + ["--gpu", "1"])
    assert rc == 0, err
    rc0, out0, err0 = run(cmd + ["--gpu", "0"])
    assert rc0 == 0, err0
    (g, how), (g0, how0) = found_n(err), found_n(err0)
    assert g == g0 and out == out0 and how.startswith("GPU kernel") and how0 == "host", (err, err0)
    a, mu, seed = oracle_best(oracle_range(fixture("4o4o4_S243_10-43_L"), 11, first, count, 1), 11, first, 1)
    assert g == (a, mu, seed - 11, seed, count, F(10), first, 1)
    rc, _, err2 = run([CHK, "-q", str(P), "-M", S243_L], stdin=out)
    assert rc == 0 and "SUCCESS" in err2, err2


def test_tool_walks_all_orders_of_ten_rows():
    """(g) the full walk of 10! orders on the device: the winner reproduces under one oracle call at the reported order and seed,
    is no worse than the best of range (f), and its program checks"""
    rc, out, err = run([OPT, "-q", str(P), "--only", "N", "-O", "1", "--seed", "11", S243_L])
    assert rc == 0, err
    (a, mu, pi, seed, count, total, first, sub), how = found_n(err)
    print(err)
    assert (count, total, first, sub) == (F(10), F(10), 0, 1) and how.startswith("GPU kernel") and seed == 11 + pi
    M = fixture("4o4o4_S243_10-43_L")
    assert M.kernel_order(kth_permutation(10, pi), 11 + pi, seed)[:2] == (a, mu)
    fa, fm, _ = oracle_best(oracle_range(M, 11, CLI_RANGE[0], CLI_RANGE[1], 1), 11, CLI_RANGE[0], 1)
    assert (a + mu, a) <= (fa + fm, fa)
    rc, _, err2 = run([CHK, "-q", str(P), "-M", S243_L], stdin=out)
    assert rc == 0 and "SUCCESS" in err2, err2
