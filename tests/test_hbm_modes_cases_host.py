"""The cases of tests/hbm_modes_cases.py, on the host: what tests/test_gpu_hbm_modes.py relies on when it runs them on the device.

For every case: the exact number of distinct coefficients; the plan fields the case is in the suite for, as the restated rules of
build_big_plan (hbm_modes_cases.plan_info) give them for its matrix and modulus; and the condition that keeps the device test honest --
on every seed it uses, the literal oracle's additions lie at least 200 (the boundary cases of group (c): 100) below the naive count, so
the common-subexpression steps, and with them the ratios, inverses and table records of the value-table modes, decide the result."""
import pytest

import hbm_modes_cases as H

RUN = [c for c in H.CASES if not c.refused]


@pytest.mark.parametrize("case", H.CASES, ids=repr)
def test_distinct_values_and_size(case):
    rp, c, v = case.csr()
    assert len(set(v)) == case.nv
    assert len(c) <= H.ENTRY_LIMIT
    assert len(case.rows) == case.m and max(c) < case.n and all(case.rows)


@pytest.mark.parametrize("case", RUN, ids=repr)
def test_plan_fields(case):
    info = case.plan_info()
    assert set(info) == set(H.INFO_FIELDS)
    assert {k: info[k] for k in case.info} == case.info
    assert info["nv"] == case.nv and info["rb"] == H._clog2(case.p)
    eager = case.plan_info(eager=True)
    assert eager["defer"] == 0 and {k: eager[k] for k in info if k not in ("defer", "pbits", "hbits")} == {k: info[k] for k in info if k not in ("defer", "pbits", "hbits")}


def test_what_the_cases_cover_together():
    I = [c.plan_info() for c in RUN]
    nomers = [i for i in I if i["mers"] == 0 and i["mode"] in (0, 1)]
    for mode in (0, 1):
        mine = [i for i in nomers if i["mode"] == mode]
        assert {i["invtab"] for i in mine} == {0, 1}
        assert {i["agg_dual"] for i in mine} == {0, 1}
        assert {7, 13, 15} <= {i["agg_cb"] for i in mine if i["agg_dual"]}
        assert {i["defer"] for i in mine} == {0, 1}
        assert 30 in {i["rb"] for i in mine}
    assert max(2 * i["bb"] + i["kb"] for i in nomers) == 48                                   # a key of all 48 bits
    assert {33, 512, 513} <= {i["nv"] for i in nomers}
    assert {(i["mode"], i["nv"]) for i in I if i["nv"] in (32, 33, 512, 513)} == {(2, 32), (1, 33), (1, 512), (0, 513)}
    assert any(i["mers"] == 17 for i in I)                                                     # the control
    assert any(i["wide"] for i in I) and any(i["idk"] for i in I)


@pytest.mark.parametrize("case", RUN, ids=repr)
def test_the_oracle_saves_additions_on_every_seed(case):
    adds, muls = H.oracle_costs(case)
    naive = H.naive_additions(case.rows)
    assert len(adds) == H.NSEEDS
    assert all(a + case.floor <= naive for a in adds), (naive, adds)


def test_agg_dual_boundary_triple_is_in_every_row():
    """(c): the triple (column 0, column 1, ratio 3) has frequency m, so its count fills the 7-bit field of the 126-row case"""
    for m in (126, 127):
        case = H.BY_NAME["c-%d-rows" % m]
        T = H.triples(case.rows, case.p)
        assert T[(0, 1, 3)] == m == max(T.values())
        assert 256 < case.plan_info()["NCmax"] <= 512
    assert 126 < (1 << 7) and H._clog2(126 + 2) == 7 and H._clog2(127 + 2) == 8


def test_far_columns_set_the_top_key_bit():
    """(d): most triples of frequency 2 and more, the most frequent among them, start at a column of 256 and more: with 9 column bits beside a 30-bit
    residue that is bit 47 of their key, bit 63 of their record"""
    for case in (c for c in H.CASES if c.name.startswith("d-")):
        info, T = case.plan_info(), H.triples(case.rows, case.p)
        freq = {k: f for k, f in T.items() if f >= 2}
        far = {k: f for k, f in freq.items() if k[0] >= 256}
        assert len(far) >= 500 and 2 * len(far) > len(freq) and max(far.values()) == max(freq.values()) >= 8
        assert info["bb"] == 9 and all(k[0] >> 8 == 1 for k in far)
        if case.p == H.P30:
            assert 2 * info["bb"] + info["kb"] == 48 and all(((k[0] << 39 | k[1] << 30 | k[2]) << 16) >> 63 == 1 for k in far)


def test_refusal_boundary():
    """(g): one more entry takes the column bound from 512 to 513"""
    a, b, c = (H.BY_NAME[k] for k in ("g-512-columns", "g-513-columns", "g-513-columns-32-values"))
    assert H.naive_additions(b.rows) == H.naive_additions(a.rows) + 1 == 974 == H.naive_additions(c.rows)
    assert sum(x != y for x, y in zip(a.rows, b.rows)) == 1
    with pytest.raises(H.Refused, match=b.refused):
        b.plan_info()
    assert c.nv <= 32 < a.nv == b.nv


def test_argmin_cases_take_one_mode_each():
    assert [H.BY_NAME[k].plan_info()["mode"] for k in H.ARGMIN] == [1, 0]
