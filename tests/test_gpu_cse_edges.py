"""The one-wave CSE kernel (plo_cse_wave.hip: run_candidate and program_gen_general through CSEPlan) on the edge cases of
tests/synth.py cse_cases(): the tie pick at 1, 2, 63 .. 66, 128 and 129 tied triples, a first step of exactly G and G + 1 rows
for every row-length class, rows of 4 .. 64 entries, one to three mask words, ProgramGen's keys filling and overflowing the
pair table they share, ProgramGen at 63 and 64 rows, 64 Triangle rows, rows of 64 general entries and more than 64 multipliers,
moduli from 3 to 2^31 - 1 and the 51-bit key.  tests/test_cse_cases_host.py holds every case to its property on the CPU.  Every
expected count comes live from the CPU oracle (oracle/plo_oracle.c), seed for seed; `best` is the argmin of the oracle's costs
under each cost mode, the smallest seed on ties."""
import pytest

import synth
from plo_testlib import OracleMatrix, oracle_chain

pytestmark = pytest.mark.gpu

CASES = synth.cse_cases()
BY = {c.name: c for c in CASES}
TABLE = {x: BY["cse_pgen_table_" + x] for x in ("a_64x1", "b_64x2", "c_20x2_44x1", "d_triangle", "e_2x2_62x1")}
FULL = [TABLE[x] for x in ("c_20x2_44x1", "d_triangle", "e_2x2_62x1")]          # ProgramGen fills their first table: the launch is repeated
HBM_SEEDS = 8
_om, _exp = {}, {}


def key(ops, seed, mode=0):
    from plinopt_amd import cmp_op_count_key
    return cmp_op_count_key(ops[0], ops[1], mode) + (seed,)


def om(c):
    if c.name not in _om:
        _om[c.name] = OracleMatrix(*(c.csr + (c.p,)))
    return _om[c.name]


def expected(c, seeds=None, seed0=0, n=0):
    """[(adds, muls)] of the oracle, each (case, seeds) computed once"""
    k = (c.name, tuple(seeds) if seeds is not None else (seed0, n))
    if k not in _exp:
        a, mu = om(c).cost_many(seeds=seeds, nthreads=8) if seeds is not None else om(c).cost_many(seed0=seed0, nseeds=n, nthreads=8)
        _exp[k] = list(zip(a, mu))
    return _exp[k]


def tiny_matrix():
    """the 3 x 3 matrix that chain_cases() pairs with the large ones"""
    if "tiny" not in _om:
        _om["tiny"] = next(x for x in synth.chain_cases() if x.name == "chain_region_big_tiny").B
    return _om["tiny"]


def plan_of(c):
    from plinopt_amd import CSEPlan
    return CSEPlan(*(c.csr + (c.p,)))


def argmin(exp, seed0, mode):
    k = min(range(len(exp)), key=lambda k: key(exp[k], seed0 + k, mode))
    return exp[k][0], exp[k][1], seed0 + k


# ---------------------------------------------------------------------------------------------------- parity and search
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_case_costs_and_argmin(hip, name):
    c = BY[name]
    plan = plan_of(c)
    assert plan.is_hbm == c.hbm                                 # what synth.wave_plan predicts
    s0, n = c.run
    if c.hbm:                                                   # the HBM family: the plan's kind and eight seeds
        ga, gm = plan.cost_many(seed0=s0, n=HBM_SEEDS)
        assert list(zip(ga, gm)) == expected(c, seed0=s0, n=HBM_SEEDS)
        plan.close()
        return
    exp = expected(c, seed0=s0, n=n)
    ga, gm = plan.cost_many(seed0=s0, n=n)
    first = plan.last_stats["launches"]
    print(name, "launches of the first call:", first)
    assert list(zip(ga, gm)) == exp
    if c.family == "pgen_table":
        assert (first == 1) if c.prop["launches"] == 1 else (first >= 2), first
    ga, gm = plan.cost_many(seeds=c.seeds)
    got = list(zip(ga, gm))
    assert got == expected(c, seeds=c.seeds) and plan.last_stats["launches"] == 1       # (the plan keeps the table that ran)
    twice = [k for k, s in enumerate(c.seeds) if c.seeds.count(s) == 2]
    assert len(twice) == 2 and got[twice[0]] == got[twice[1]]
    for mode in (0, 1, 2):
        assert plan.search(s0, n, mode) == argmin(exp, s0, mode), mode                  # mode 2: the winner's split, not (sum, 0)
        assert plan.last_stats["launches"] == 1
    plan.close()


@pytest.mark.parametrize("name", ["cse_tie_unit_T65", "cse_pgen_shape_gen64x6"])
def test_search_over_1_3_5_257_candidates(hip, name):
    c = BY[name]
    s0 = 7
    exp = expected(c, seed0=s0, n=257)
    plan = plan_of(c)
    for cnt in (1, 3, 5, 257):
        for mode in (0, 1, 2):
            assert plan.search(s0, cnt, mode) == argmin(exp[:cnt], s0, mode), (cnt, mode)
    assert len({argmin(exp[:cnt], s0, 0) for cnt in (1, 3, 5, 257)}) >= 2                # (the winner moves with the count)
    plan.close()


# ---------------------------------------------------------------------------------------------------- -E
@pytest.mark.parametrize("name", [c.name for c in CASES if c.enum])
def test_schedule_walk(hip, name):
    """every step of these cases offers 63, 64 or 65 and more children: rem % T, rem /= T and the saturating product on the tie list"""
    c = BY[name]
    plan = plan_of(c)
    for first in (0, synth.CSE_ENUM_FAR):
        exp = om(c).enum_cost_many(first, c.enum, nthreads=8)
        assert plan.enum_cost_many(first, c.enum) == tuple(exp), first
        assert max(exp[2]) == 2 ** 64 - 1
    exp = om(c).enum_cost_many(0, c.enum, nthreads=8)
    best, maxprod = plan.enum_search(0, c.enum, 1)
    k = min(range(c.enum), key=lambda k: (exp[0][k], exp[1][k], k))
    assert best == (exp[0][k], exp[1][k], k) and maxprod == max(exp[2])
    plan.close()


# ---------------------------------------------------------------------------------------------------- ProgramGen and the table
def test_programgen_fills_the_table_exactly(hip):
    """64 keys in 64 slots, 128 in 128: no slot is empty when tab_find runs, and nothing is repeated"""
    for x in ("a_64x1", "b_64x2"):
        c = TABLE[x]
        plan = plan_of(c)
        ga, gm = plan.cost_many(seed0=0, n=8)
        assert set(zip(ga, gm)) == {c.prop["costs"]} and plan.last_stats["launches"] == 1
        assert plan.search(0, 8) == c.prop["costs"] + (0,) and plan.last_stats["launches"] == 1
        plan.close()


@pytest.mark.parametrize("name", [c.name for c in FULL])
def test_programgen_overflow_repeats_every_entry(hip, name):
    """a fresh plan per entry: the first table is full inside ProgramGen (pass A1, or Triangle's insertion into `multiples`),
    the launch is repeated with twice the slots, and the plan keeps them"""
    c = BY[name]
    exp = expected(c, seed0=0, n=8)
    for mode in (0, 1, 2):
        plan = plan_of(c)
        assert plan.search(0, 8, mode) == argmin(exp, 0, mode)
        print(name, "search mode", mode, "launches", plan.last_stats["launches"])
        assert plan.last_stats["launches"] >= 2
        assert plan.search(0, 8, mode) == argmin(exp, 0, mode) and plan.last_stats["launches"] == 1
        plan.close()
    want = om(c).enum_cost_many(0, 4, nthreads=4)
    plan = plan_of(c)
    assert plan.enum_cost_many(0, 4) == tuple(want)
    print(name, "enum_cost_many launches", plan.last_stats["launches"])
    assert plan.last_stats["launches"] >= 2
    best, maxprod = plan.enum_search(0, 4, 1)
    assert best == (want[0][0], want[1][0], 0) and maxprod == max(want[2]) and plan.last_stats["launches"] == 1
    plan.close()
    plan = plan_of(c)
    best, maxprod = plan.enum_search(0, 4, 1)
    assert best == (want[0][0], want[1][0], 0) and maxprod == max(want[2]) and plan.last_stats["launches"] >= 2
    plan.close()


@pytest.mark.parametrize("name", [c.name for c in FULL])
def test_programgen_overflow_in_a_chain(hip, name):
    """as the first and as the second matrix of a chained candidate: the chain's repeat doubles both tables"""
    from plinopt_amd import CSEChain
    c = BY[name]
    tiny = tiny_matrix()
    assert c.p == synth.CHAIN_PRIME
    T = OracleMatrix(*(tiny.csr + (c.p,)))
    for A, B, OA, OB in ((c, tiny, om(c), T), (tiny, c, T, om(c))):
        ch = CSEChain(A.csr, B.csr, c.p)
        ga, gm = ch.cost_many(seed0=0, n=8)
        assert list(zip(ga, gm)) == [oracle_chain(OA, OB, s) for s in range(8)]
        print(name, "first" if A is c else "second", "chain launches", ch.last_stats["launches"])
        assert ch.last_stats["launches"] >= 2
        ga, gm = ch.cost_many(seed0=0, n=8)
        assert list(zip(ga, gm)) == [oracle_chain(OA, OB, s) for s in range(8)] and ch.last_stats["launches"] == 1
        ch.close()
