"""Edge-shape parity of the change-of-basis kernels (plo_cob.hip, host side plo_capi.hip) against the references of
tests/cob_cases.py: more than 64 coefficients (the table kernel's later trips and idle lanes), indices next to 2^32, the switch
between the table kernel and the generic one and their LDS limits, batches of unequal problems, the threshold encoding, small
and large moduli, coefficients that are not residues.  Every check runs on the table kernel and, with PLO_COB_GENERIC=1 (read
per call), on the generic one; the references are computed once per case and shared (tests/test_cob_cases_host.py checks them
and the properties of these inputs on the CPU)."""
import pytest

import cob_cases as cc

pytestmark = pytest.mark.gpu
KERNELS = pytest.mark.parametrize("generic", [False, True], ids=["table", "generic"])
by_name = lambda cases: pytest.mark.parametrize("case", cases, ids=[c.name for c in cases])


def select(monkeypatch, generic):
    if generic:
        monkeypatch.setenv("PLO_COB_GENERIC", "1")
    else:
        monkeypatch.delenv("PLO_COB_GENERIC", raising=False)


def problem(c, w0=-1, w1=-1):
    return (c.TM, c.Cand, c.coeffs, c.p, w0, w1)


def refused(code, call, *a, **kw):
    from plinopt_amd import capi
    with pytest.raises(capi.PloError) as e:
        call(*a, **kw)
    assert e.value.code == code, e.value


# ------------------------------------------------------------------------------------------ (a) across the wave width
@KERNELS
@by_name(cc.wave_width_cases())
def test_whole_enumeration_across_the_wave_width(hip, monkeypatch, generic, case):
    from plinopt_amd import cob_search
    select(monkeypatch, generic)
    got, st = cob_search(*cc.args(case))
    assert got == cc.whole_ref(case)
    assert st["candidates"] == len(case.coeffs) ** 4 and st["launches"] == 1


# ------------------------------------------------------------------------------------------ (b) slices
@KERNELS
@by_name(cc.slice_cases())
def test_slices_equal_the_slice_reference(hip, monkeypatch, generic, case):
    from plinopt_amd import capi, cob_search
    select(monkeypatch, generic)
    C = len(case.coeffs)
    for k, (g0, gn) in enumerate(cc.slices_of(C)):
        w0, w1 = cc.slice_thresholds(case, k)
        got, st = cob_search(*cc.args(case), w0, w1, groups=(g0, gn))
        assert got == cc.slice_ref(case, w0, w1, g0, gn), (g0, gn, w0, w1)
        assert st["candidates"] == gn * C
        if gn == 0:
            assert got == (w0, w1, 0, 0)
    for g0, gn in ((C ** 3, 1), (C ** 3 - 1, 2), (C ** 3 + 1, 0), (0, C ** 3 + 1), (1 << 40, 1)):
        refused(capi.PLO_E_ARG, cob_search, *cc.args(case), groups=(g0, gn))


# ------------------------------------------------------------------------------------------ (c) planted winners
@pytest.mark.parametrize("generic,case,exp", cc.planted_cases(), ids=[("generic-" if g else "table-") + c.name for g, c, _ in cc.planted_cases()])
def test_planted_winner_of_a_whole_enumeration(hip, monkeypatch, generic, case, exp):
    """255^4 = 4.2e9 candidates on the table kernel (index up to 2^32 - 66 716 671), 129^4 on the generic one"""
    from plinopt_amd import cob_search
    select(monkeypatch, generic)
    C = len(case.coeffs)
    assert cc.lds_model(C, case.m, 4 - case.row, generic)[1] == (not generic)
    got, st = cob_search(*cc.args(case))
    print("%s: kernel %.3f ms, call %.3f s" % (case.name, st["kernel_ms"], st["seconds"]))
    assert got == exp
    assert st["candidates"] == C ** 4 and st["lds_bytes"] == cc.lds_model(C, case.m, 4 - case.row, generic)[0]


# ------------------------------------------------------------------------------------------ (d) kernel switch and LDS limits
@KERNELS
@by_name(cc.switch_cases())
def test_switch_between_the_table_kernel_and_the_generic_one(hip, monkeypatch, generic, case):
    from plinopt_amd import cob_search, cob_search_batch
    select(monkeypatch, generic)
    C, qn = len(case.coeffs), cc.qn_row0(case.n, case.off)
    lds, tab = cc.lds_model(C, case.m, qn, generic)
    assert tab == (not generic and case.m < 654)
    exp = cc.whole_ref(case)
    got, st = cob_search(*cc.args(case))
    assert got == exp and st["lds_bytes"] == lds
    g = exp[2] // C
    got, st = cob_search(*cc.args(case), groups=(g, C ** 3 - g))
    assert got == exp and st["lds_bytes"] == lds and st["candidates"] == C ** 4 - g * C
    got, st = cob_search_batch(case.n, case.m, case.row, case.off, [problem(case)])
    assert got == [exp] and st["lds_bytes"] == lds


@KERNELS
def test_generic_kernel_lds_limit(hip, monkeypatch, generic):
    """C = 3, n = 4, row 0: the largest m whose 4 x m block, 4 x 4 nullspace block and 3 coefficients fit the 160 KiB cap runs and
    equals the oracle on the three entry points; one more column is refused by all three"""
    from plinopt_amd import capi, cob_search, cob_search_batch
    select(monkeypatch, generic)
    m = cc.generic_limit_m(3, 4)
    fit = cc.rand_case("limit-m%d" % m, 31, 3, 4, m, 0, cc.P17)
    over = cc.rand_case("limit-m%d" % (m + 1), 32, 3, 4, m + 1, 0, cc.P17)
    lds, tab = cc.lds_model(3, m, 4, generic)
    assert not tab and lds <= cc.LDS_CAP < lds + 16
    exp = cc.whole_ref(fit)
    got, st = cob_search(*cc.args(fit))
    assert got == exp and st["lds_bytes"] == lds
    got, st = cob_search(*cc.args(fit), groups=(0, 27))
    assert got == exp and st["lds_bytes"] == lds
    got, st = cob_search_batch(4, m, 0, 0, [problem(fit), problem(fit, 0, -1)])
    assert got == [exp, cc.whole_ref(fit, 0, -1)] and st["lds_bytes"] == lds
    refused(capi.PLO_E_CAPACITY, cob_search, *cc.args(over))
    refused(capi.PLO_E_CAPACITY, cob_search, *cc.args(over), groups=(3, 2))
    refused(capi.PLO_E_CAPACITY, cob_search_batch, 4, m + 1, 0, 0, [problem(over)])


# ------------------------------------------------------------------------------------------ (e) thresholds
@KERNELS
@by_name(cc.threshold_cases())
def test_thresholds_follow_the_lexicographic_order(hip, monkeypatch, generic, case):
    from plinopt_amd import cob_search, cob_search_batch
    select(monkeypatch, generic)
    C = len(case.coeffs)
    zv, zw, idx, found = cc.whole_ref(case)
    assert found
    thr = cc.thresholds_around(zv, zw, case.n)
    assert ((zv, -1, 1) in thr) == (zw == 0)
    g0 = max(idx // C - 1, 0)
    for w0, w1, fnd in thr:
        exp = cc.whole_ref(case, w0, w1)
        assert exp == ((zv, zw, idx, 1) if fnd else (w0, w1, 0, 0))
        got, _ = cob_search(*cc.args(case), w0, w1)
        assert got == exp, (w0, w1)
        got, _ = cob_search(*cc.args(case), w0, w1, groups=(g0, 3))
        assert got == cc.slice_ref(case, w0, w1, g0, 3) == exp, (w0, w1)
    for part in (thr[:4], thr[4:]):
        got, _ = cob_search_batch(case.n, case.m, case.row, case.off, [problem(case, w0, w1) for w0, w1, _ in part])
        assert got == [cc.whole_ref(case, w0, w1) for w0, w1, _ in part], part


# ------------------------------------------------------------------------------------------ (f) moduli and values
def _moduli(prefix):
    return by_name([c for c in cc.moduli_cases() if c.name.startswith(prefix)])


def _whole_slices_batch(case):
    """the whole enumeration, its two halves reduced, and a batch of two thresholds against the oracle"""
    from plinopt_amd import cob_search, cob_search_batch
    C = len(case.coeffs)
    exp = cc.whole_ref(case)
    got, st = cob_search(*cc.args(case))
    assert got == exp and st["candidates"] == C ** 4
    h = C ** 3 // 2
    parts = [cob_search(*cc.args(case), groups=g)[0] for g in ((0, h), (h, C ** 3 - h))]
    assert cc.reduce_shards(parts, case.n, -1, -1) == exp
    thr = [(-1, -1), (exp[0], exp[1] - 1), (exp[0], exp[1]), (0, -1)]
    got, _ = cob_search_batch(case.n, case.m, case.row, case.off, [problem(case, *w) for w in thr])
    assert got == [cc.whole_ref(case, *w) for w in thr]


@KERNELS
@_moduli("mod")
def test_small_moduli_with_colliding_coefficients(hip, monkeypatch, generic, case):
    """p = 3: 0, 1, -1, 2, -2 are 0, 1, 2, 2, 1 -- equal rows at different indices resolve to the smallest index"""
    select(monkeypatch, generic)
    _whole_slices_batch(case)


@KERNELS
@_moduli("max")
def test_largest_operands_of_31_bit_moduli(hip, monkeypatch, generic, case):
    """every entry of TM, of the chosen rows and every coefficient is p-1: four summands (p-1)^2 per column"""
    select(monkeypatch, generic)
    _whole_slices_batch(case)


@KERNELS
@_moduli("multiples")
def test_coefficients_that_are_multiples_of_the_modulus(hip, monkeypatch, generic, case):
    """coefficients p and 2p are zeros of w, p+1 is 1: counted on residues, as the oracle does"""
    select(monkeypatch, generic)
    assert case.p in case.coeffs and 2 * case.p in case.coeffs and 2 * case.p < 2 ** 32
    _whole_slices_batch(case)


# ------------------------------------------------------------------------------------------ (g) batches of unequal problems
@KERNELS
@pytest.mark.parametrize("batch", cc.batch_sets(), ids=[b[0] for b in cc.batch_sets()])
def test_batch_of_unequal_problems(hip, monkeypatch, generic, batch):
    """one launch whose grid is that of the largest problem, every blockIdx.y with its own range; a problem whose chosen rows are
    dependent is not launched; one problem that does not fit the tables sends the whole batch to the generic kernel"""
    from plinopt_amd import cob_search, cob_search_batch
    select(monkeypatch, generic)
    name, n, m, row, off, probs = batch
    exp = [cc.whole_ref(c) for c in probs]
    got, st = cob_search_batch(n, m, row, off, [problem(c) for c in probs])
    assert got == exp
    assert st["launches"] == 1 and st["candidates"] == sum(len(c.coeffs) ** 4 for c in probs)
    live = [c for c in probs if not c.name.endswith("dependent")]
    assert len(live) == (3 if name == "dependent" else 4) and all(e[3] for c, e in zip(probs, exp) if c in live)
    qn = cc.qn_row0(n, off) - row                      # (row 0: the block's unit vectors; row 1 at n = 4: the 3-dimensional complement of one row)
    models = [cc.lds_model(len(c.coeffs), m, qn, generic) for c in live]
    tab = all(t for _, t in models)
    assert tab == (not generic and name != "fallback")
    if name == "fallback":
        assert [t for _, t in (cc.lds_model(len(c.coeffs), m, qn, False) for c in live)] == [True, False, True, True]
    assert st["lds_bytes"] == max(cc.lds_model(len(c.coeffs), m, qn, generic or not tab)[0] for c in live)
    largest = max(live, key=lambda c: len(c.coeffs))
    _, one = cob_search(*cc.args(largest))
    if tab == cc.lds_model(len(largest.coeffs), m, qn, generic)[1]:
        assert st["grid"] == one["grid"]               # sized from the largest problem, as its own call
    # the same problems in another order give the same results
    got, _ = cob_search_batch(n, m, row, off, [problem(c) for c in reversed(probs)])
    assert got == exp[::-1]
