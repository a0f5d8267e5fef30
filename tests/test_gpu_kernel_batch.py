"""plo_kernel_batch_search (plo_kmethod_batch.hip: the kernel method on many matrices, one workgroup per problem, one minimum
each) against the C oracle: for every problem of every batch the cost AND the seed of the minimum of
OracleMatrix.kernel_restart over its own seeds seed0 + q*per .. + per-1, bit for bit, and status 0.  Problems are the edge
shapes of synth.kmethod_cases() at KM_PRIME and window matrices of 3x4x7_63_rational_L.slp.  PLO_BATCH_GRID=1 makes one
workgroup take every problem of a launch in turn (what another plan left in LDS must not be read); PLO_KMETHOD_PAIRS_DIV and
PLO_KMETHOD_ENT_DIV undersize Dep's image of the sampled problems, which only those may repeat."""
import os
from types import SimpleNamespace

import pytest

import pruner_lib as pl
import synth
from plo_testlib import DATA, FieldP, OracleMatrix

pytestmark = pytest.mark.gpu

P = synth.KM_PRIME
GRID = "PLO_BATCH_GRID"
INF = (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 64 - 1)
KM = {c.name: c for c in synth.kmethod_cases()}
_exp = {}


def prob(name, n, rows, p=P):
    rows = [{j: v % p for j, v in r.items() if v % p} for r in rows]
    m = len(rows)
    csr = (m, n) + synth.to_csr(rows, p)
    R = synth.rank_mod(rows, p)
    return SimpleNamespace(name=name, m=m, n=n, rows=rows, p=p, csr=csr, O=OracleMatrix(*(csr + (p,))), rank=R, ndeps=m - R,
                           unit=all(v in (1, p - 1) for r in rows for v in r.values()), refusal=synth.km_refusal(m, n, rows, p))


def case(name):
    c = KM[name]
    assert c.p == P
    return prob(name, c.n, c.rows)


def quiet(x):
    """hard bound of Dep's pairs at most 32: such a problem can never fill the 64 slots every table has at least"""
    return x.ndeps * x.rank * (x.rank - 1) // 2 <= 32


def key(ops, seed, mode=0):
    a, mu = ops
    return ((a + mu, a), (a, mu), (a + mu,))[mode] + (seed,)


def expected(x, seed0, per, mode=0):
    """(adds, muls, seed) of the oracle's minimum under (cost key of mode, seed) over the restarts seed0 .. seed0+per-1"""
    out = []
    for s in range(seed0, seed0 + per):
        if (x.name, s) not in _exp:
            _exp[(x.name, s)] = x.O.kernel_restart(s)[:2]
        out.append(_exp[(x.name, s)])
    j = min(range(per), key=lambda j: key(out[j], seed0 + j, mode))
    return out[j] + (seed0 + j,)


def check(probs, per, seed0=0, mode=0):
    from plinopt_amd import kernel_batch_search
    bests, status, st = kernel_batch_search([x.csr for x in probs], P, seed0, per, cost_mode=mode)
    for q, x in enumerate(probs):
        exp = expected(x, seed0 + q * per, per, mode)
        print(q, x.name, "unit" if x.unit else "general", status[q], bests[q], exp)
    for q, x in enumerate(probs):
        assert status[q] == 0 and bests[q] == expected(x, seed0 + q * per, per, mode), (q, x.name)
    return st


@pytest.fixture(scope="module")
def windows():
    """the nine windows over three variables of 3x4x7_63_rational_L.slp (7x6 to 14x13; each has a kernel)"""
    text = open(os.path.join(DATA, "3x4x7_63_rational_L.slp")).read()
    out = []
    for w in pl.windows(text, singles=False, only=["t26", "b76", "e1"]):
        m, n = len(w["outs"]), len(w["ins"])
        _, _, rp, c, v = pl.csr_of(pl.window_matrix(w, FieldP(P)), m, n)
        rows = [{c[k]: v[k] for k in range(rp[i], rp[i + 1])} for i in range(m)]
        out.append(prob("window_" + "_".join(w["sel"]), n, rows))
    assert len(out) == 9 and all(x.refusal is None for x in out)
    return out


@pytest.fixture(scope="module")
def mixed(windows):
    """Unit and general problems alternating while both last, the unit ones from the smallest up and the general ones from the
    largest down: under PLO_BATCH_GRID=1 a workgroup meets a large problem after a small one and a small one after a large one"""
    names = ["km_a_4x2", "km_a_64x32", "km_a_68x34", "km_a_127x64", "km_a_128x64", "km_a_64x32_vals", "km_b_65x1", "km_b_66x2", "km_b_68x4", "km_b_40x3_rank1",
             "km_c_R4_ones", "km_c_R5_1toR", "km_c_R8_ones", "km_c_R9_1toR", "km_c_R16_ones", "km_c_R17_1toR", "km_c_R32_1toR", "km_c_R33_ones", "km_c_R64_ones",
             "km_c_64x16_dense", "km_d_15x8_3empty", "km_d_3x2_empty", "km_d_dup_unit", "km_d_dup_twice", "km_d_12x16_even", "km_f_112x56"]
    every = [case(n) for n in names] + windows + [prob("2x1", 1, [{0: 1}, {0: 1}])]
    assert all(x.refusal is None for x in every)
    size = lambda x: x.m * (x.n + x.rank)     # noqa: E731
    u, g = sorted([x for x in every if x.unit], key=size), sorted([x for x in every if not x.unit], key=size, reverse=True)
    out = []
    while u or g:
        if u:
            out.append(u.pop(0))
        if g:
            out.append(g.pop(0))
    assert len(out) >= 30 and sum(1 for a, b in zip(out, out[1:]) if a.unit != b.unit) >= 12
    assert any({} in x.rows for x in out) and any(x.m > 64 for x in out)
    return out


@pytest.mark.parametrize("per", [1, 2, 3, 5, 7])
def test_one_problem_fewer_restarts_than_waves(hip, windows, per):
    """per_problem below, and no multiple of, the waves of a workgroup: a wave without a restart must not reach the result"""
    st = check([windows[4]], per, seed0=2 ** 40 + 5)
    assert st["candidates"] == per and st["grid"] == 1 and 1 <= st["launches"] <= 2
    assert st["waves_per_wg"] <= per * 2


@pytest.mark.parametrize("grid", [None, "1"])
def test_mixed_batch(hip, monkeypatch, mixed, grid):
    if grid:
        monkeypatch.setenv(GRID, grid)
    per = 5
    st = check(mixed, per, seed0=7)
    extra, loud = st["candidates"] - len(mixed) * per, sum(1 for x in mixed if not quiet(x))
    print("launches", st["launches"], "extra candidates", extra)
    assert extra >= 0 and extra % per == 0 and extra <= 5 * per * loud      # (a table of 0.75 x the sampled pairs may fill: that problem alone is run again)
    assert st["launches"] >= 4                         # the sizing launch and one per bucket: 4x2 and 128x64 are classes apart
    if grid:
        assert st["grid"] == 1


def test_the_same_matrix_at_three_positions(hip, mixed):
    """the 4x2 block: every restart costs the same, so the winner is each range's first seed"""
    from plinopt_amd import kernel_batch_search
    w = case("km_a_4x2")
    probs, per = [w, mixed[3], w, mixed[8], mixed[9], w], 23
    bests, status, _ = kernel_batch_search([x.csr for x in probs], P, 0, per)
    got = [bests[q] for q in (0, 2, 5)]
    for q, b in zip((0, 2, 5), got):
        assert b == expected(w, q * per, per) and q * per <= b[2] < (q + 1) * per
    assert len({b[:2] for b in got}) == 1 and len({b[2] for b in got}) == 3
    assert status == [0] * 6


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_cost_modes(hip, mixed, mode):
    small = sorted([x for x in mixed if not x.unit], key=lambda x: x.m)[:6]
    assert len(small) == 6
    check(small, 11, seed0=3, mode=mode)


def test_refused_problems_between_problems_that_fit(hip, windows):
    from plinopt_amd import capi, kernel_batch_search
    bad = ["km_refuse_4x7_fullrank", "km_refuse_3x2_allempty", "km_refuse_129x2", "km_refuse_3x65", "km_refuse_67x2_65dep", "km_refuse_65x3_a2"]
    want = ["PLO_E_UNSUPPORTED"] * 5 + ["PLO_E_CAPACITY"]
    probs = [windows[0]]
    for k, name in enumerate(bad):
        c = KM[name]
        assert c.refusal == want[k] == synth.km_refusal(c.m, c.n, c.rows, c.p)
        probs += [SimpleNamespace(name=name, csr=c.csr, refusal=c.refusal), windows[k + 1]]
    per = 5
    bests, status, st = kernel_batch_search([x.csr for x in probs], P, 0, per)
    for q, x in enumerate(probs):
        if x.refusal:
            assert status[q] == getattr(capi, x.refusal) and bests[q] == INF, x.name
        else:
            assert status[q] == 0 and bests[q] == expected(x, q * per, per), x.name
    assert st["candidates"] == 7 * per


@pytest.mark.parametrize("knob,value", [("PLO_KMETHOD_PAIRS_DIV", "8"), ("PLO_KMETHOD_ENT_DIV", "4")])
def test_only_the_problems_short_of_room_are_run_again(hip, monkeypatch, mixed, knob, value):
    """15x8_3empty and 12x16_even: Dep has up to 7 and 4 rows of 8 entries with values all over Z_p, 28 distinct triples a row -- the
    64 slots that an eighth of the sampled pairs asks for do not hold three such rows.  68x4: Dep has up to 64 rows of up to 4
    entries -- a quarter of the sampled entries does not hold its rows.  (All three are sampled: their hard-bound images are larger
    than the wave's region.)  The quiet problems keep their one launch.  64x16_dense is not here: its M has so many triples that the
    scale 16 its Dep would need under PAIRS_DIV no longer fits M's own table into the LDS (PLO_E_CAPACITY, as plo_kernel_search)."""
    q_ = [x for x in mixed if quiet(x)][:6]
    loud = [case("km_d_15x8_3empty"), case("km_b_68x4"), case("km_d_12x16_even")]
    assert len(q_) == 6 and not any(quiet(x) for x in loud)
    probs, per = q_[:3] + [loud[0]] + q_[3:5] + [loud[1], loud[2]] + q_[5:], 6
    st0 = check(probs, per, seed0=11)
    monkeypatch.setenv(knob, value)
    st = check(probs, per, seed0=11)
    extra = st["candidates"] - len(probs) * per
    print("launches", st0["launches"], "->", st["launches"], "extra candidates", extra)
    assert st["launches"] > st0["launches"]
    assert extra > 0 and extra % per == 0 and extra <= 5 * per * len(loud)


def test_agreement_with_the_single_problem_entry(hip, mixed):
    from plinopt_amd import kernel_batch_search, kernel_search
    probs, per, seed0 = [case("km_a_68x34"), case("km_a_64x32_vals"), mixed[6]], 9, 2 ** 33
    bests, status, _ = kernel_batch_search([x.csr for x in probs], P, seed0, per)
    for q, x in enumerate(probs):
        assert status[q] == 0 and bests[q] == kernel_search(x.csr, P, seed0 + q * per, per, per_block=1, want_costs=False)[3], x.name
