"""The edge-shape family of the one-wave CSE kernel (tests/synth.py cse_cases) against the host-side model and the CPU oracle
alone: every case must have, from its matrix, the property it was built for -- the number of triples of maximal frequency, the
rows of the first step against the rows of a trip, ProgramGen's keys against the slots of the pair table, the mask words, the
row-length class -- and the cases meant to tell a wrong pick from a right one must show several costs over their seeds,
otherwise tests/test_gpu_cse_edges.py could pass on a wrong kernel.  No GPU."""
import time

import synth
from plo_testlib import OracleMatrix

CASES = synth.cse_cases()
BY = {c.name: c for c in CASES}
FAMILIES = {"tie": 12, "group": 23, "rowlen": 19, "mw": 6, "pgen_table": 5, "pgen_shape": 7, "moduli": 17}
_scores = {}


def fam(f):
    return [c for c in CASES if c.family == f]


def all_seeds(c):
    return [c.run[0] + k for k in range(c.run[1])] + c.seeds


def scores(c):
    """[(adds, muls)] of the oracle over the case's run and list, computed once"""
    if c.name not in _scores:
        a, mu = OracleMatrix(*(c.csr + (c.p,))).cost_many(seeds=all_seeds(c))
        _scores[c.name] = list(zip(a, mu))
    return _scores[c.name]


def test_cases_are_deterministic():
    again = synth.cse_cases()
    assert [(c.name, c.family, c.m, c.n, c.p, c.csr, c.run, c.seeds, c.enum, c.hbm, c.sha256) for c in again] == \
           [(c.name, c.family, c.m, c.n, c.p, c.csr, c.run, c.seeds, c.enum, c.hbm, c.sha256) for c in CASES]
    assert len(set(BY)) == len(CASES) and {f: len(fam(f)) for f in FAMILIES} == FAMILIES and len(CASES) == sum(FAMILIES.values())


def test_matrices_are_valid_csr_and_seed_lists_hold_the_edges():
    for c in CASES:
        m, n, rp, col, val = c.csr
        assert (m, n) == (c.m, c.n) and len(rp) == m + 1 and rp[0] == 0 and rp[-1] == len(col) == len(val)
        for i in range(m):
            row = col[rp[i]:rp[i + 1]]
            assert row == sorted(set(row)) and all(0 <= j < n for j in row)
        assert all(0 < v < c.p for v in val)
        if not c.hbm:
            assert {2 ** 64 - 1, 2 ** 63} <= set(c.seeds) and any(2 ** 40 < s < 2 ** 63 for s in c.seeds) and len(set(c.seeds)) == len(c.seeds) - 1
        assert c.run[1] >= 8


def test_wave_plan_agrees_with_the_stated_refusal():
    sent = [c.name for c in CASES if c.hbm]
    assert sent == ["cse_rowlen_L65_unit", "cse_moduli_key53_8x1023"]
    for c in CASES:
        plan = synth.wave_plan(c.m, c.n, c.rows, c.p)
        assert isinstance(plan, str) == c.hbm and (plan == "PLO_E_CAPACITY" if c.hbm else plan.cap == c.plan.cap), c.name
    # with at most 32 distinct coefficients the HBM family takes what the wave kernel refuses
    assert all(len({v for r in c.rows for v in r.values()}) <= 32 for c in CASES if c.hbm)
    k53 = BY["cse_moduli_key53_8x1023"]
    assert max(len(r) for r in k53.rows) == 2 and k53.n == 1023          # refused for the key alone: 2 * 11 + 31 bits


def test_tie_counts_at_maximal_frequency():
    """recomputed from the matrix: a tie count that drifts fails here"""
    unit = {c.T: c for c in fam("tie") if c.plan.unit}
    gen = {c.T: c for c in fam("tie") if not c.plan.unit}
    assert sorted(unit) == [1, 2, 63, 64, 65, 66, 128, 129] and sorted(gen) == [63, 64, 65, 66]
    for c in fam("tie"):
        t = synth.cse_triples(c.rows, c.p)
        mf = max(t.values())
        assert (mf, sum(v == mf for v in t.values())) == (c.maxfreq, c.T), c.name
        assert c.run == synth.CSE_TIE_RUN
        # -E: the children of the root are the triples of frequency >= 2; at maximal frequency 2 these are the tied ones
        if c.enum:
            assert c.T in (63, 64, 65) and c.maxfreq == 2 and sum(v >= 2 for v in t.values()) == c.T
    assert sorted(c.T for c in fam("tie") if c.enum) == [63, 63, 64, 64, 65, 65]
    assert [c.name for c in CASES if c.enum and c.family != "tie"] == []


def test_group_cases_sit_on_the_rows_of_a_trip():
    seen = set()
    for c in fam("group"):
        L = c.maxlen
        assert c.G == 64 >> max(2, (L - 1).bit_length())
        held = [i for i, r in enumerate(c.rows) if 0 in r and 1 in r]
        if L < 64:
            t = synth.cse_triples(c.rows, c.p)
            (key, f), = [(k, v) for k, v in t.items() if v >= 2]             # one triple repeats: the first step is forced
            assert key[:2] == (0, 1) and f == c.prop["share"] and len(held) == c.prop["mask"], c.name
            assert c.prop["share"] - c.G in (-1, 0, 1) and (c.prop["mask"] - c.prop["share"] == (0 if c.plan.unit else 1))
            assert all(len(r) == L for r in c.rows)
            seen.add((L, c.plan.unit, c.prop["share"] - c.G))
        else:
            assert c.G == 1 and len(held) == c.m == c.prop["share"] and all(len(r) == 64 for r in c.rows)
    for L in (4, 8, 16, 32):
        assert {(L, True, 0), (L, True, 1), (L, False, 0), (L, False, 1)} <= seen
    assert {(L, False, -1) for L in (4, 8, 16)} <= seen                      # the one-trip path with a row that is not rewritten
    assert sorted((c.m, c.plan.unit) for c in fam("group") if c.maxlen == 64) == [(2, False), (2, True), (3, False), (3, True)]


def test_rowlen_cases_cover_every_class_boundary():
    got = sorted((c.maxlen, c.plan.unit) for c in fam("rowlen") if not c.hbm)
    assert got == sorted((L, u) for L in (4, 5, 8, 9, 16, 17, 32, 33, 64) for u in (False, True))
    for c in fam("rowlen"):
        if c.hbm:
            assert c.maxlen == 65
            continue
        assert c.lpr_log2 == max(2, (c.maxlen - 1).bit_length()) and c.G == 64 >> c.lpr_log2
        assert c.G == 1 or c.m % c.G, c.name                                # a partial last trip of the r0 += G loops
    assert {c.maxlen: c.lpr_log2 for c in fam("rowlen") if not c.hbm} == {4: 2, 5: 3, 8: 3, 9: 4, 16: 4, 17: 5, 32: 5, 33: 6, 64: 6}


def test_mw_cases_cover_the_mask_words():
    assert sorted((c.m, c.plan.mw) for c in fam("mw")) == [(63, 1), (64, 1), (65, 2), (100, 2), (128, 2), (129, 3)]
    assert all(c.plan.unit for c in fam("mw"))
    c = BY["cse_mw_straddle_100x7"]
    held = [i for i, r in enumerate(c.rows) if 0 in r and 1 in r]
    assert c.top == [(0, 1, 1)] and c.maxfreq == len(held) == 40                 # the first step is forced and rewrites these rows
    assert sum(i < 64 for i in held) > c.G and 63 in held and 64 in held and sum(i >= 64 for i in held) >= 2


def test_pgen_table_keys_against_slots():
    a, b, c, d, e = (BY["cse_pgen_table_" + x] for x in ("a_64x1", "b_64x2", "c_20x2_44x1", "d_triangle", "e_2x2_62x1"))
    for x in (a, b, c, d, e):
        assert x.maxfreq <= 1 and x.m == 64 and not x.plan.unit               # no CSE step: the pair table is ProgramGen's from the start
        assert x.keys == len(synth.cse_pgen_keys(x.rows, x.p))
    assert (a.keys, a.plan.cap) == (64, 64) and (b.keys, b.plan.cap) == (128, 128)                   # exactly full
    assert (c.keys, c.plan.cap) == (84, 64) and (e.keys, e.plan.cap) == (66, 64)                     # pass A1 overflows
    assert (d.keys, d.plan.cap) == (128, 128)                                                          # full after A1; Triangle's key is one more
    for x, launches in ((c, 2), (d, 2), (e, 2)):                                                       # the model of the repeat: twice the slots hold the keys
        assert x.prop["launches"] == launches and synth.wave_plan(x.m, x.n, x.rows, x.p, cap_scale=4).cap == 2 * x.plan.cap >= x.keys + 1
    # the oracle's costs, on every seed
    for x in (a, b, c, e):
        assert set(scores(x)) == {x.prop["costs"]}, x.name
    assert len(set(scores(d))) == 1
    # d differs from b's pattern by the couple of column 0 alone: Triangle saves nothing there but one multiplication moves
    assert scores(d)[0][0] == 64


def test_pgen_shape_cases():
    for name in ("cse_pgen_shape_gen63x6", "cse_pgen_shape_gen64x6"):
        assert len(set(scores(BY[name]))) >= 3, (name, set(scores(BY[name])))
    assert max(mu for _, mu in scores(BY["cse_pgen_shape_mult66_blocks"])) > 64
    t = BY["cse_pgen_shape_triangle_64"]
    assert all(len(r) == 2 and 0 in r for r in t.rows) and len({min(r[0], t.p - r[0]) for r in t.rows}) == 64
    # Triangle's `found` is never reset: the couple (2, 4) is not looked at; with rows 3 and 4 exchanged it is the first couple left
    n = BY["cse_pgen_shape_triangle_found"]
    assert set(scores(n)) == {n.prop["costs"]} == {(5, 6)}
    swapped = [n.rows[i] for i in (0, 1, 2, 4, 3)]
    a, mu = OracleMatrix(n.m, n.n, *synth.to_csr(swapped, n.p), n.p).cost_many(seed0=0, nseeds=2)
    assert set(zip(a, mu)) == {(5, 5)}
    f = BY["cse_pgen_shape_factor_rows_2x64"]
    assert set(synth.cse_triples(f.rows, f.p).values()) == {1}
    # FactorOutRows alone works on it: 63 additions per row less one per collapsed |v| ... the rows end with 8 entries each
    assert set(scores(f)) == {(2 * 63, 2 * 8)}, set(scores(f))


def test_moduli_cases():
    assert sorted(c.p for c in fam("moduli") if c.m == 10) == sorted(synth.CSE_MODULI * 2)
    assert all((c.m, c.n) == (10, 7) for c in fam("moduli") if "key" not in c.name)
    assert [c.plan.unit for c in fam("moduli") if c.name.startswith("cse_moduli_gen_")] == [p == 3 for p in synth.CSE_MODULI]
    for name in ("cse_moduli_key51_8x1022", "cse_moduli_key51_8x1000"):
        c = BY[name]
        assert c.plan.NC == 1024 and 2 * 10 + (c.p - 1).bit_length() == 51
    assert BY["cse_moduli_key51_8x1000"].maxfreq >= 2


def test_oracle_scores_every_case_quickly_and_the_tie_cases_vary():
    t0 = time.time()
    for c in CASES:
        for a, mu in scores(c):
            assert 0 <= a < 1 << 16 and 0 <= mu < 1 << 16, c.name
        s = scores(c)
        assert s[len(s) - 1] == s[len(s) - 2] or c.hbm                       # the seed given twice
    for c in fam("tie"):
        assert len(set(scores(c))) >= 3, (c.name, sorted(set(scores(c))))
    enum = 0
    for c in CASES:
        if c.enum:
            O = OracleMatrix(*(c.csr + (c.p,)))
            for first in (0, synth.CSE_ENUM_FAR):
                a, mu, prod = O.enum_cost_many(first, c.enum)
                assert max(prod) == 2 ** 64 - 1, c.name                       # the product of the radices saturates
                enum += len(set(zip(a, mu)))
    took = time.time() - t0
    print("oracle: %d cases, %.2f s, %d distinct enumerated costs" % (len(CASES), took, enum))
    assert took < 30
