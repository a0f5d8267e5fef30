"""The chained-candidate kernels (plo_cse_wave.hip: cse_chain_kernel through CSEChain, cse_chain_batch_kernel through
chain_batch) on the synthetic edge cases of tests/synth.py chain_cases(): both orders of a pair, the four unit/general
dispatches, first matrices that draw nothing from the random stream, a large image before a tiny one and the reverse, more
than 64 rows, rows of 64 entries, moduli 3 to 2^31 - 1, one wave per workgroup, and the documented refusals.  Every expected
count comes live from the CPU oracle (oracle/plo_oracle.c plo_oracle_chain), seed for seed; `best` is the oracle's argmin under
each cost mode.

The second half takes the table-full relaunch of the wave family on purpose (PLO_WAVE_CAP_TIGHT): the first pair
table just holds the initial triples, a candidate whose live triples grow fills it, the device reports that and the host
repeats the launch with twice the slots -- run_job (plan search, cost_many, the -E enumeration), run_chain and the loop of
plo_cse_chain_batch.  Each test asserts that the repeat happened and that the results are the oracle's."""
import ctypes
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import synth
from plo_testlib import OracleMatrix, oracle_chain

pytestmark = pytest.mark.gpu

CASES = synth.chain_cases()
BY = {c.name: c for c in CASES}
ADMITTED = [c for c in CASES if not c.refusal]
REFUSED = [c for c in CASES if c.refusal]
_mats, _exp = {}, {}


def key(ops, seed, mode=0):
    from plinopt_amd import cmp_op_count_key
    return cmp_op_count_key(ops[0], ops[1], mode) + (seed,)


def mats(c):
    if c.name not in _mats:
        _mats[c.name] = [OracleMatrix(*(x.csr + (c.p,))) for x in (c.A, c.B)]
    return _mats[c.name]


def pair(c):
    return (c.A.csr, c.B.csr)


def expected(todo):
    """oracle_chain of every (case, seed) of todo, each computed once per session, the missing ones eight at a time"""
    miss = sorted({(c.name, s) for c, s in todo if (c.name, s) not in _exp})
    for name in {name for name, _ in miss}:
        mats(BY[name])
    with ThreadPoolExecutor(max_workers=8) as ex:
        for k, v in zip(miss, ex.map(lambda ns: oracle_chain(*(mats(BY[ns[0]]) + [ns[1]])), miss)):
            _exp[k] = v
    return [_exp[(c.name, s)] for c, s in todo]


# ---------------------------------------------------------------------------------------------------- one pair per plan
@pytest.mark.parametrize("name", [c.name for c in ADMITTED])
def test_chain_case_costs_and_argmin(hip, name):
    from plinopt_amd import CSEChain
    c = BY[name]
    s0, n = c.run
    run = [s0 + k for k in range(n)]
    exp = expected([(c, s) for s in run])
    ch = CSEChain(c.A.csr, c.B.csr, c.p)
    ga, gm = ch.cost_many(seed0=s0, n=n)
    assert list(zip(ga, gm)) == exp
    launches = 2 if c.relaunch else 1                           # (the 150 x 6 table fills up under the usual sizing)
    assert ch.last_stats["launches"] == launches
    plans = [synth.wave_plan(x.m, x.n, x.rows, c.p, cap_scale=2 * launches) for x in (c.A, c.B)]
    assert (ch.last_stats["waves_per_wg"], ch.last_stats["lds_bytes"]) == synth.chain_layout(*plans)
    assert c.relaunch or synth.chain_layout(*plans) == (c.waves, c.lds)
    if c.family == "onewave":
        assert ch.last_stats["waves_per_wg"] == 1
    ga, gm = ch.cost_many(seeds=c.seeds)
    assert list(zip(ga, gm)) == expected([(c, s) for s in c.seeds])
    for mode in (0, 1, 2):
        k = min(range(n), key=lambda k: key(exp[k], run[k], mode))
        assert ch.search(s0, n, mode) == (exp[k][0], exp[k][1], run[k]), mode      # mode 2: the winner's split, not (sum, 0)
    ch.close()


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("name", [c.name for c in REFUSED])
def test_refused_pair_raises_its_code(hip, name):
    from plinopt_amd import CSEChain, capi, chain_batch
    c = BY[name]
    with pytest.raises(capi.PloError) as e:
        CSEChain(c.A.csr, c.B.csr, c.p)
    assert e.value.code == getattr(capi, c.refusal) and "LDS-resident" in str(e.value)
    ok = BY["chain_dispatch_unit_gen_6"]
    with pytest.raises(capi.PloError) as e:
        chain_batch([pair(ok), pair(c), pair(ok)], c.p, 0, 2)
    assert e.value.code == getattr(capi, c.refusal) and "pair 1:" in str(e.value)


def test_argument_errors(hip):
    from plinopt_amd import CSEChain, capi, chain_batch
    ok = BY["chain_dispatch_unit_gen_6"]
    L = capi.lib()
    csr, keep = capi.make_csr(*ok.A.csr)
    h = ctypes.c_void_p()
    for first, second, out in ((None, ctypes.byref(csr), ctypes.byref(h)), (ctypes.byref(csr), None, ctypes.byref(h)), (ctypes.byref(csr), ctypes.byref(csr), None)):
        assert L.plo_cse_chain_create(first, second, ok.p, out) == capi.PLO_E_ARG
    assert not h.value
    for pairs, per_pair, mode in (([pair(ok)], 0, 0), ([], 3, 0), ([pair(ok)], 3, 3)):
        with pytest.raises(capi.PloError) as e:
            chain_batch(pairs, ok.p, 0, per_pair, cost_mode=mode)
        assert e.value.code == capi.PLO_E_ARG
    ch = CSEChain(ok.A.csr, ok.B.csr, ok.p)
    with pytest.raises(capi.PloError) as e:
        ch.search(0, 8, 3)
    assert e.value.code == capi.PLO_E_ARG
    ch.close()


# ---------------------------------------------------------------------------------------------------- many pairs per launch
def launches_of(per_pair):
    """The admitted cases in batch launches: all of one modulus together, shuffled so that large and small pairs alternate (the
    dense 60 x 60 one stays out: the oracle's second per seed; so do the two whose table fills up, see below); and those of the main modulus whose regions leave four waves to
    a workgroup once more on their own, since the large ones put the launch of all on one wave per workgroup."""
    out = []
    for p in [synth.CHAIN_PRIME] + synth.CHAIN_MODULI:
        cs = [c for c in ADMITTED if c.p == p and c.family != "onewave" and not c.relaunch]
        random.Random(0xBA7C4 + per_pair).shuffle(cs)
        out.append((p, cs))
        if p == synth.CHAIN_PRIME:
            out.append((p, [c for c in cs if c.family in ("order", "dispatch", "silent", "mw")]))
    return out


def batch_waves(cs):
    """(waves per workgroup, LDS bytes) as plo_cse_chain_batch lays a launch out: the first of 4, 2, 1 waves that fits"""
    region = max(x.region_bytes for c in cs for x in c.plans)
    rsmax = max(x.rs_bytes for c in cs for x in c.plans)
    return next((w, 64 + w * (2 * rsmax + region)) for w in (4, 2, 1) if 64 + w * (2 * rsmax + region) <= synth.LDS_MAX)


def check_batch(cs, p, per_pair, seed0):
    from plinopt_amd import chain_batch
    n = len(cs) * per_pair
    exp = expected([(cs[k // per_pair], seed0 + k) for k in range(n)])
    ga, gm, best, st = chain_batch([pair(c) for c in cs], p, seed0, per_pair)
    assert list(zip(ga, gm)) == exp, next((cs[k // per_pair].name, seed0 + k) for k in range(n) if (ga[k], gm[k]) != exp[k])
    b = min(range(n), key=lambda k: key(exp[k], seed0 + k))
    assert best == (exp[b][0], exp[b][1], seed0 + b)
    assert st["launches"] == 1 and st["candidates"] == n
    assert (st["waves_per_wg"], st["lds_bytes"]) == batch_waves(cs)
    return exp, st


@pytest.mark.parametrize("seed0", [0, 2 ** 40])
@pytest.mark.parametrize("per_pair", [1, 3, 11])
def test_batch_of_all_cases_of_a_modulus(hip, per_pair, seed0):
    from plinopt_amd import chain_batch
    four = 0
    for p, cs in launches_of(per_pair):
        assert len(cs) >= 2
        exp, st = check_batch(cs, p, per_pair, seed0)
        four += st["waves_per_wg"] == 4
        # sum-only keys: (sum, 0) and the smallest seed of that sum; no costs asked for
        ga, gm, best, st = chain_batch([pair(c) for c in cs], p, seed0, per_pair, cost_mode=2, want_costs=False)
        b = min(range(len(exp)), key=lambda k: key(exp[k], seed0 + k, 2))
        assert ga is None and gm is None and best == (exp[b][0] + exp[b][1], 0, seed0 + b) and st["launches"] == 1
    assert four >= 4                                            # counts that do not divide the waves of a workgroup were among them


def test_batch_of_one_pair(hip):
    for name in ("chain_order_u8x6_g7x5", "chain_mw_128x4_129x4"):
        check_batch([BY[name]], BY[name].p, 5, 3)


def test_batch_with_the_dense_60x60_pair(hip):
    """one wave per workgroup in the batch kernel: the 130 KB region next to a pair of a few hundred bytes"""
    cs = [BY["chain_onewave_60x60_tiny"], BY["chain_silent_freq1_first"]]
    _, st = check_batch(cs, synth.CHAIN_PRIME, 1, 0)
    assert st["waves_per_wg"] == 1


# ---------------------------------------------------------------------------------------------------- grid stride
def test_grid_stride_loop_turns_twice(hip):
    """More candidates than resident waves: every wave's region is used again, in the batch by a pair of another size"""
    from plinopt_amd import CSEChain, chain_batch
    small, other = BY["chain_order_u8x6_g7x5"], BY["chain_dispatch_gen_unit_12"]
    ch = CSEChain(small.A.csr, small.B.csr, small.p)
    ch.cost_many(seed0=0, n=1 << 20)
    st = ch.last_stats
    assert st["grid"] * st["waves_per_wg"] < 1 << 20            # the launch was as wide as the device takes
    n = 2 * st["grid"] * st["waves_per_wg"] + 3
    ga, gm = ch.cost_many(seed0=7, n=n)
    assert ch.last_stats["grid"] == st["grid"]
    assert list(zip(ga, gm)) == expected([(small, 7 + k) for k in range(n)])
    k = min(range(n), key=lambda k: key((ga[k], gm[k]), 7 + k))
    assert ch.search(7, n) == (ga[k], gm[k], 7 + k)
    ch.close()
    cs = [small, other]
    _, _, _, st = chain_batch([pair(c) for c in cs], small.p, 0, 1 << 19, want_costs=False)
    per_pair = st["grid"] * st["waves_per_wg"] + 2              # 2 per_pair candidates: the loop turns twice, the pair changes inside a turn
    assert 2 * per_pair < 1 << 20
    exp, st2 = check_batch(cs, small.p, per_pair, 11)
    assert st2["grid"] == st["grid"]


# ---------------------------------------------------------------------------------------------------- the table-full relaunch
TIGHT = "PLO_WAVE_CAP_TIGHT"


def dense(seed, m, n, vals, p=synth.CHAIN_PRIME):
    """(OracleMatrix, csr tuple, rows) of a dense m x n matrix over vals"""
    _, rows = synth._dense(random.Random(seed), m, n, vals)
    csr = (m, n) + synth.to_csr(rows, p)
    return OracleMatrix(*(csr + (p,))), csr, rows


# the smallest of the dense few-valued matrices tried whose live triples outgrow the tight table on the device (their initial
# triples sit just under a power of two) and fit twice that: +-1, and three-valued for ProgramGen's general path
def tight_unit():
    return dense(0x7161, 12, 11, [1, -1])


def tight_general():
    return dense(0x7162, 16, 10, [1, -1, 2])


def tight_plans(rows, m, n):
    """the plan of the first launch under the knob and the plan that must have followed it"""
    first, second = (synth.wave_plan(m, n, rows, synth.CHAIN_PRIME, cap_scale=s, tight=True) for s in (2, 4))
    assert first.distinct < first.cap <= 2 * first.distinct and second.cap == 2 * first.cap
    return first, second


@pytest.mark.parametrize("which", ["unit", "general"])
def test_plan_search_and_cost_many_after_a_full_table(hip, monkeypatch, which):
    from plinopt_amd import CSEPlan
    O, csr, rows = tight_unit() if which == "unit" else tight_general()
    exp = O.cost_many(seed0=0, nseeds=8, nthreads=8)
    plain = CSEPlan(*(csr + (O.p,)))
    assert tuple(plain.cost_many(seed0=0, n=8)) == tuple(exp) and plain.last_stats["launches"] == 1
    want = {mode: plain.search(0, 8, mode) for mode in (0, 1, 2)}
    assert want[0] == O.search(0, 8, 0, nthreads=8)
    plain.close()
    monkeypatch.setenv(TIGHT, "1")
    plan = CSEPlan(*(csr + (O.p,)))
    assert tuple(plan.cost_many(seed0=0, n=8)) == tuple(exp)
    print("CSEPlan.cost_many", which, "launches", plan.last_stats["launches"])
    assert plan.last_stats["launches"] >= 2
    plan.close()
    for mode in (0, 1, 2):
        plan = CSEPlan(*(csr + (O.p,)))                         # a fresh plan: the table starts tight again
        assert plan.search(0, 8, mode) == want[mode]
        print("CSEPlan.search", which, mode, "launches", plan.last_stats["launches"])
        assert plan.last_stats["launches"] >= 2
        plan.close()


def test_schedule_enumeration_after_a_full_table(hip, monkeypatch):
    from plinopt_amd import CSEPlan
    O, csr, rows = tight_unit()
    n = 48
    exp = O.enum_cost_many(0, n, nthreads=8)
    monkeypatch.setenv(TIGHT, "1")
    plan = CSEPlan(*(csr + (O.p,)))
    assert plan.enum_cost_many(0, n) == tuple(exp)
    print("CSEPlan.enum_cost_many launches", plan.last_stats["launches"])
    assert plan.last_stats["launches"] >= 2
    plan.close()
    plan = CSEPlan(*(csr + (O.p,)))
    best, maxprod = plan.enum_search(0, n, 1)
    k = min(range(n), key=lambda k: (exp[0][k], exp[1][k], k))
    assert best == (exp[0][k], exp[1][k], k) and maxprod == max(exp[2])
    print("CSEPlan.enum_search launches", plan.last_stats["launches"])
    assert plan.last_stats["launches"] >= 2
    plan.close()


def test_chain_after_a_full_table(hip, monkeypatch):
    from plinopt_amd import CSEChain
    (A, acsr, arows), (B, bcsr, brows) = tight_general(), tight_unit()
    exp = [oracle_chain(A, B, s) for s in range(8)]
    monkeypatch.setenv(TIGHT, "1")
    ch = CSEChain(acsr, bcsr, A.p)
    ga, gm = ch.cost_many(seed0=0, n=8)
    st = ch.last_stats
    print("CSEChain.cost_many launches", st["launches"])
    assert list(zip(ga, gm)) == exp and st["launches"] >= 2
    # both plans were rebuilt with twice the slots, and chain_config ran on them
    plans = [tight_plans(rows, csr[0], csr[1]) for rows, csr in ((arows, acsr), (brows, bcsr))]
    scale = 1 << (st["launches"] - 1)
    last = [synth.wave_plan(csr[0], csr[1], rows, A.p, cap_scale=2 * scale, tight=True) for rows, csr in ((arows, acsr), (brows, bcsr))]
    assert st["lds_bytes"] >= max(x.region_bytes for x in last) > max(x[0].region_bytes for x in plans)
    assert (st["waves_per_wg"], st["lds_bytes"]) == synth.chain_layout(*last)
    ch.close()
    for mode in (0, 1, 2):
        ch = CSEChain(acsr, bcsr, A.p)
        k = min(range(8), key=lambda k: key(exp[k], k, mode))
        assert ch.search(0, 8, mode) == (exp[k][0], exp[k][1], k)
        print("CSEChain.search", mode, "launches", ch.last_stats["launches"])
        assert ch.last_stats["launches"] >= 2
        ch.close()


def test_chain_batch_after_a_full_table(hip, monkeypatch):
    """four pairs, only the third fills its table: every plan of the launch is rebuilt"""
    from plinopt_amd import chain_batch
    (A, acsr, _), (B, bcsr, _) = tight_unit(), tight_general()
    quiet = [BY[n] for n in ("chain_dispatch_unit_gen_6", "chain_silent_1x1_first", "chain_dispatch_gen_gen_6")]
    pairs = [pair(quiet[0]), pair(quiet[1]), (acsr, bcsr), pair(quiet[2])]
    om = [mats(quiet[0]), mats(quiet[1]), [A, B], mats(quiet[2])]
    per_pair, seed0 = 3, 2 ** 40
    exp = [oracle_chain(*(om[k // per_pair] + [seed0 + k])) for k in range(4 * per_pair)]
    monkeypatch.setenv(TIGHT, "1")
    for c in quiet:                                             # these fit their tight tables: alone they run once
        assert chain_batch([pair(c)], c.p, seed0, per_pair)[3]["launches"] == 1
    ga, gm, best, st = chain_batch(pairs, A.p, seed0, per_pair)
    print("chain_batch launches", st["launches"])
    assert list(zip(ga, gm)) == exp and st["launches"] >= 2
    b = min(range(len(exp)), key=lambda k: key(exp[k], seed0 + k))
    assert best == (exp[b][0], exp[b][1], seed0 + b)


def test_the_knob_changes_nothing_when_unset(hip, monkeypatch):
    from plinopt_amd import CSEChain
    monkeypatch.delenv(TIGHT, raising=False)
    c = BY["chain_region_big_tiny"]
    ch = CSEChain(c.A.csr, c.B.csr, c.p)
    ch.cost_many(seed0=0, n=2)
    assert (ch.last_stats["launches"], ch.last_stats["lds_bytes"]) == (1, c.lds)
    ch.close()


# ---------------------------------------------------------------------------------------------------- tables that cannot grow
def test_relaunch_keeps_the_tables_that_cannot_grow(hip):
    """The device's error word does not say whose table was full, so the host doubles every table of the launch.  One that no
    longer fits the LDS with twice the slots must keep the table that ran (the full one may be another's) and not turn the
    call into a refusal: the 150 x 6 matrix, whose 64 slots fill up under the usual sizing, next to matrices of 8192 slots."""
    from plinopt_amd import CSEChain, chain_batch
    full, big, long_ = BY["chain_mw_150x6_gen"], BY["chain_region_big_tiny"], BY["chain_rowlen_2x64_gen"]
    p = full.p
    A, B = full.A, long_.A
    assert synth.wave_plan(B.m, B.n, B.rows, p).cap == 8192 and synth.wave_plan(B.m, B.n, B.rows, p, cap_scale=4) == "PLO_E_CAPACITY"
    ch = CSEChain(A.csr, B.csr, p)
    ga, gm = ch.cost_many(seed0=0, n=4)
    assert list(zip(ga, gm)) == [oracle_chain(mats(full)[0], mats(long_)[0], s) for s in range(4)]
    st = ch.last_stats
    print("CSEChain.cost_many, 150x6 before 2x64: launches", st["launches"])
    assert st["launches"] == 2
    assert (st["waves_per_wg"], st["lds_bytes"]) == synth.chain_layout(synth.wave_plan(A.m, A.n, A.rows, p, cap_scale=4), synth.wave_plan(B.m, B.n, B.rows, p))
    ch.close()
    cs, per_pair = [big, full, long_], 2
    exp = expected([(cs[k // per_pair], k) for k in range(len(cs) * per_pair)])
    ga, gm, best, st = chain_batch([pair(c) for c in cs], p, 0, per_pair)
    print("chain_batch, 40x32 / 150x6 / 2x64: launches", st["launches"])
    assert list(zip(ga, gm)) == exp and st["launches"] == 2
    b = min(range(len(exp)), key=lambda k: key(exp[k], k))
    assert best == (exp[b][0], exp[b][1], b)


def test_a_full_table_that_cannot_grow_is_refused_and_the_plan_stays_usable(hip):
    """Dense 64 x 64 +-1: 8192 slots that fill up (the live triples grow to 2.2 times the initial 4032) and cannot be doubled
    inside the LDS.  Every entry answers PLO_E_CAPACITY, and answers it again: the plan is not left half built."""
    from plinopt_amd import CSEChain, CSEPlan, capi, chain_batch
    _, csr, rows = dense(0x7164, 64, 64, [1, -1])
    p = synth.CHAIN_PRIME
    assert synth.wave_plan(64, 64, rows, p).cap == 8192 and synth.wave_plan(64, 64, rows, p, cap_scale=4) == "PLO_E_CAPACITY"
    tiny = BY["chain_region_big_tiny"].B.csr
    plan, ch = CSEPlan(*(csr + (p,))), CSEChain(tiny, csr, p)
    assert not plan.is_hbm
    for call in (lambda: plan.cost_many(seed0=0, n=2), lambda: plan.search(0, 2), lambda: ch.cost_many(seed0=0, n=2), lambda: ch.search(0, 2),
                 lambda: chain_batch([(csr, tiny), (tiny, tiny)], p, 0, 1)) * 2:
        with pytest.raises(capi.PloError) as e:
            call()
        assert e.value.code == capi.PLO_E_CAPACITY and "pair table full" in str(e.value)
    plan.close()
    ch.close()
