"""tests/cob_cases.py against the C oracle alone: the slice reference and the planted-winner builder compute what the oracle
computes, and the inputs of tests/test_gpu_cob_edges.py have the properties that make them tell a wrong kernel from a right one
(winners past lane 63 of the table kernel's first trip, winners at indices next to 2^32).  No GPU."""
import random

import pytest

import cob_cases as cc
from plo_testlib import oracle_cob_search

THRESHOLDS = lambda rng, n, m: rng.choice([(-1, -1), (0, -1), (m // 2, -1), (m // 2, 0), (m // 3, n), (m // 3, n + 1), (-1, 3), (1, 1)])


def _random_cases():
    rng = random.Random(2024)
    for t in range(30):
        p = rng.choice([3, 7, 101, cc.P17, cc.PA, cc.PM])
        n, C, m = rng.randint(1, 7), rng.randint(1, 9), rng.randint(1, 12)
        row = rng.randint(0, n - 1)
        kind = ["unit", "random", "dependent"][t % 3]
        coeffs = cc.good_last(C, p) if t % 2 else cc.usual_coeffs(C, p)
        yield cc.rand_case("host-%d" % t, t, C, n, m, row, p, coeffs=coeffs, chosen=kind, wide=bool(t % 4 == 0)), THRESHOLDS(rng, n, m)


def test_ref_range_over_the_whole_range_is_the_oracle():
    found = dependent = 0
    for c, (w0, w1) in _random_cases():
        C = len(c.coeffs)
        exp = oracle_cob_search(*cc.args(c), w0, w1)
        assert cc.ref_range(*cc.args(c), w0, w1, 0, C ** 3) == exp, c.name
        found += exp[3]
        dependent += int(c.name[5:]) % 3 == 2 and c.row > 0     # (chosen rows that admit no candidate)
        assert exp[3] == 0 or not (int(c.name[5:]) % 3 == 2 and c.row > 0)
    assert found >= 10 and dependent >= 5


def test_union_of_slices_is_the_whole():
    rng = random.Random(5)
    for c, (w0, w1) in _random_cases():
        C = len(c.coeffs)
        cuts = sorted({0, C ** 3} | {rng.randrange(C ** 3 + 1) for _ in range(3)})
        parts = [cc.ref_range(*cc.args(c), w0, w1, a, b - a) for a, b in zip(cuts, cuts[1:])]
        assert cc.reduce_shards(parts, c.n, w0, w1) == oracle_cob_search(*cc.args(c), w0, w1), c.name


def test_coefficient_orders():
    for p in (cc.P17, cc.PA):
        assert cc.good_last(7, p) == [3, p - 3, 2, p - 2, 1, p - 1, 0]
        assert cc.good_last(6, p, zero=False) == [3, p - 3, 2, p - 2, 1, p - 1]
        for C in (1, 2, 64, 65, 255):
            for z in (True, False):
                assert sorted(cc.good_last(C, p, z)) == sorted(cc.usual_coeffs(C, p, z)) and len(set(cc.good_last(C, p, z))) == C


@pytest.mark.parametrize("C", [9, 16, 24])
@pytest.mark.parametrize("row", [0, 1])
def test_planted_winner_is_the_oracles(C, row):
    for p, idx4 in ((cc.P17, (1, C // 2, 2, C - 1)), (cc.PA, (C - 1, 0, C - 2, 3)), (cc.P17, (C - 1, C - 1, 1, C - 1))):
        c, exp = cc.planted(C, p, idx4, row)
        assert oracle_cob_search(*cc.args(c)) == exp, c.name
        assert exp[0] == c.m and exp[2] <= ((idx4[0] * C + idx4[1]) * C + idx4[2]) * C + idx4[3]


def test_whole_enumerations_past_64_coefficients_win_in_a_later_trip():
    """every whole enumeration with C >= 65 has its winner at l >= 64: a table kernel that stops after its first trip of 64 lanes,
    or mishandles the idle lanes of the last one, cannot find it"""
    big = [c for c in cc.wave_width_cases() if len(c.coeffs) >= 65]
    assert len(big) >= 3
    for c in big:
        zv, zw, idx, found = cc.whole_ref(c)
        assert found and idx % len(c.coeffs) >= 64, c.name
    for generic, c, exp in cc.planted_cases():
        assert len(c.coeffs) >= 65 and exp[3] and exp[2] % len(c.coeffs) >= 64, c.name
    for name, n, m, row, off, probs in cc.batch_sets():
        assert [len(c.coeffs) for c in probs] in ([65, 3, 64, 1], [3, 7, 5, 1])
        assert all((c.n, c.m, c.row, c.off) == (n, m, row, off) for c in probs)


def test_planted_targets_sit_at_the_ends_of_the_index():
    seen = set()
    for generic, c, exp in cc.planted_cases():
        C = len(c.coeffs)
        name = c.name.split("-")[-1].split("_")
        seen |= {("l", generic)} if int(name[3]) == C - 1 else set()
        seen |= {("i", generic)} if int(name[0]) == C - 1 else set()
        assert {c.p for g, c, e in cc.planted_cases() if g == generic} == {cc.P17, cc.PA}
        assert {c.row for g, c, e in cc.planted_cases() if g == generic} == {0, 1}
    assert seen == {("l", False), ("l", True), ("i", False), ("i", True)}


def test_slices_reach_the_top_of_the_index_and_cover_the_shapes():
    cases = cc.slice_cases()
    assert {len(c.coeffs) for c in cases} == {65, 128, 129, 255} and {c.n for c in cases} == {1, 4, 5, 6, 7}
    assert {min(4, c.n - c.off) for c in cases} == {1, 2, 3, 4}
    top = 0
    for c in cases:
        C = len(c.coeffs)
        sl = cc.slices_of(C)
        assert {gn for _, gn in sl} >= {0, 1, 3, 4, 5, 9} and (0, 3) in sl and (C ** 3 - 3, 3) in sl and (C * C - 2, 4) in sl
        assert all(gn * C <= 9 * 255 for _, gn in sl)
        if C == 255:
            k = sl.index((C ** 3 - 3, 3))
            res = cc.slice_ref(c, *cc.slice_thresholds(c, k), *sl[k])
            top += res[3] and res[2] >= 2 ** 32 - 2 ** 26
    assert top >= 1


def test_threshold_cases_have_the_winners_they_are_named_for():
    a, b = cc.threshold_cases()
    za, zb = cc.whole_ref(a), cc.whole_ref(b)
    assert za[3] and za[0] >= 1 and za[1] >= 1
    assert zb[3] and zb[0] >= 1 and zb[1] == 0 and 0 not in b.coeffs and b.n == 4
    for c, (zv, zw, idx, _) in ((a, za), (b, zb)):
        for w0, w1, fnd in cc.thresholds_around(zv, zw, c.n):
            exp = oracle_cob_search(*cc.args(c), w0, w1)
            assert exp[3] == fnd, (c.name, w0, w1)
            assert exp == ((zv, zw, idx, 1) if fnd else (w0, w1, 0, 0))


def test_lds_model_at_the_switch():
    ms = [c.m for c in cc.switch_cases()]
    assert ms == [652, 653, 654]
    assert [cc.lds_model(7, m, 4, False) for m in ms] == [(16 * 4606, True), (16 * 4606, True), ((4 * 654 + 16 + 7) * 4, False)]
    assert cc.lds_model(7, 652, 4, True) == ((4 * 652 + 16 + 7) * 4, False)
    m = cc.generic_limit_m(3, 4)
    assert (4 * m + 16 + 3) * 4 <= cc.LDS_CAP < (4 * (m + 1) + 16 + 3) * 4 and not cc.lds_model(3, m, 4, False)[1]
