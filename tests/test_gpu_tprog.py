"""The in-place trilinear program check on the GPU (plo_tprog.hip, plo_tprog_*, bin/TPchecker --gpu 1) against the host loop and
the independent definition of tests/tprog_cases.py: (violated, first, value, expected) must be the definition's exactly through
the ctypes mirror, and the tool's text its own --gpu 0 text.  The shapes put nb on both sides of the wave width and of two
waves, na = 1, the -e width, w at the plan's limit and one above it (from plan_info), pair ranges that cut lane blocks, and
launches of one wave each (PLO_TPROG_WAVES)."""
import math
import os
import subprocess

import pytest

import tprog_cases as C
from plo_testlib import DATA, ROOT, read_sms

pytestmark = pytest.mark.gpu

MODULI = (3, 15, 131071, C.P31)
CASES = C.edge_cases("issue") + C.edge_cases("units") + [m for m, _ in C.mutations()] + [m for m, _ in C.mutations(C.schoolbook(3, 5, True, "units"))] + [C.hidden_defect()]
TRILPLACER = os.path.join(ROOT, "bin", "trilplacer")


def plan_of(case, q):
    from plinopt_amd import TProgPlan
    return TProgPlan(*case.csr(), case.records(), q, expanded=case.expanded, matmul=case.matmul)


def device(case, q, pair0=0, pair1=None, plan=None):
    plan = plan or plan_of(case, q)
    info = plan.info()
    assert info["w"] == case.w and info["npairs"] == case.na * case.nb and info["lds_words_per_wave"] == 64 * case.w
    assert max(case.na, case.nb, case.w) <= info["max_words"] and info["waves_per_wg"] * 256 * case.w <= 160 * 1024
    naxpy = sum(r[1] == C.AXPY for r in case.records())
    assert info["rows"] == naxpy + (case.L[0] if not case.matmul else case.na * math.isqrt(case.nb * case.nc0 // case.na))
    assert info["records"] >= naxpy + (0 if case.matmul else len(case.P[2]) * (2 if case.expanded else 1))
    v, first, value, exp = plan.check(pair0, pair1)
    assert plan.last_stats["candidates"] == C.nequations(case, pair0, pair1)
    return (v, first, value, exp) if v else (0, None, None, None)


def same(case, q, pair0=0, pair1=None, plan=None):
    want = C.definition(case, q, pair0, pair1)
    assert device(case, q, pair0, pair1, plan) == want
    return want


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_device_equals_definition(hip, case):
    from plinopt_amd import capi
    for q in MODULI:
        try:
            C.definition(case, q)
        except C.Refused:
            with pytest.raises(capi.PloError) as r:
                plan_of(case, q)
            assert r.value.code == -1
            assert "no unit modulo %d" % q in str(r.value)
            continue
        same(case, q)


def tool_lines(err):
    """what must be the same text on both paths: everything but the timing line"""
    return [ln for ln in err.splitlines() if not ln.startswith("# GPU:") and not ln.startswith("# host:")]


@pytest.mark.parametrize("k", range(len(CASES)), ids=lambda k: CASES[k].name)
def test_the_tool_on_the_device_says_what_its_host_loop_says(hip, k, tmp_path):
    """every case through bin/TPchecker --gpu 1 over Q (the prime loop, the failing prime, the equation once more over Q, the
    certificate and pass lines) and modulo one of the four moduli, taken in turn over the cases (a tool run costs
    the start of the device, so not every case runs with every modulus here; the mirror test above does that)"""
    case = CASES[k]
    paths = case.write(tmp_path)
    for q in (0, MODULI[k % 4]):
        opts = case.flags() + (["-q", q] if q else []) + ["--count"]
        rc0, err0 = C.tool(opts + paths, 0)
        rc1, err1 = C.tool(opts + paths, 1)
        try:
            want = C.definition(case, q)
        except C.Refused:
            assert rc0 == rc1 == 4 and tool_lines(err0) == tool_lines(err1) and "is not invertible modulo %d" % q in err1
            continue
        assert rc0 == rc1 == (1 if want[0] else 0)
        assert tool_lines(err0) == tool_lines(err1) and "# GPU: " in err1 and "# host: " in err0
        assert "the device refuses" not in err1
        if q == 0:
            assert C.cert_of(err0) == C.cert_of(err1) and C.passes_of(err0) == C.passes_of(err1) and len(C.passes_of(err1)) >= 1
        if want[0]:
            assert C.first_of(err1) == (want[1], case.where(want[1]), str(want[2]), str(want[3]))
            if q:
                assert C.count_of(err1) == (want[0], C.nequations(case))
        if "hidden" in case.name and q == 0:
            assert [t for _, _, _, t in C.passes_of(err1)] == ["no violated equation", "violated"] and "SUCCESS" not in err1


def test_every_modulus_goes_through_the_tool_on_the_device():
    """the rotation above: each of the four moduli meets a case that it does not refuse, correct ones and mutations"""
    for q in MODULI:
        ran = []
        for k, case in enumerate(CASES):
            if MODULI[k % 4] == q:
                try:
                    ran.append(C.definition(case, q)[0])
                except C.Refused:
                    pass
        assert 0 in ran and any(v > 0 for v in ran), q


def test_the_choice_by_size_takes_the_device(hip, tmp_path):
    """without --gpu, above the crossover (PLO_TPCHECKER_CROSSOVER, a test knob), the device runs; below it the host loop"""
    case = C.mutations()[0][0]
    paths = case.write(tmp_path)
    want = C.definition(case, 131071)
    rc, err = C.tool(["-q", 131071, "--count"] + paths, None, env={"PLO_TPCHECKER_CROSSOVER": "1"})
    assert rc == 1 and "# GPU: " in err and "--gpu not given" not in err and C.first_of(err)[0] == want[1] and C.count_of(err)[0] == want[0]
    rc, err = C.tool(["-q", 131071, "--count"] + paths, None)
    assert rc == 1 and "# host: " in err and "below the crossover" in err and C.first_of(err)[0] == want[1]


def test_walking_every_record_gives_the_same(hip, monkeypatch):
    """PLO_TPROG_SKIP=0: the bilinear kernel walks the ADD and SCA records of slots that are still zero instead of passing them over"""
    monkeypatch.setenv("PLO_TPROG_SKIP", "0")
    for case in (two_far_defects(), two_far_defects(65, True), C.mutations()[8][0], C.schoolbook(2, 129, True, "units")):
        same(case, C.P31)
        same(case, 15 if "units" in case.name else 131071)


def two_far_defects(nb=129, expanded=False):
    """the schoolbook program of 2 x nb without its first and its last AXPY: violations in the first and the last wave"""
    base = C.schoolbook(2, nb, expanded)
    lines = base.text.splitlines()
    ax = [n for n, ln in enumerate(lines) if " * " in ln and ("hig" not in ln)]
    keep = [ln for n, ln in enumerate(lines) if n not in (ax[0], ax[-1])]
    return base.with_text(base.name + "_far", "\n".join(keep) + "\n")


def test_pair_ranges_that_cut_lane_blocks(hip):
    case = two_far_defects()
    assert C.definition(case)[0] >= 2
    plan = plan_of(case, 131071)
    n = 2 * 129
    for p0, p1 in ((0, n), (0, 1), (1, 2), (5, 7), (63, 65), (64, 128), (100, 130), (129, 130), (130, 200), (200, n), (n - 1, n), (1, n - 1)):
        same(case, 131071, p0, p1, plan)
    assert C.definition(case, 131071, 0, 1)[0] >= 1 and C.definition(case, 131071, n - 1, n)[0] >= 1 and C.definition(case, 131071, 1, n - 1)[0] == 0


def test_launches_of_one_wave(hip, monkeypatch, tmp_path):
    """PLO_TPROG_WAVES = 1: 2 x 3 bilinear launches behind the linear one; the first violated equation is still the global minimum
    and the count the total"""
    monkeypatch.setenv("PLO_TPROG_WAVES", "1")
    for case in (two_far_defects(), two_far_defects(65, True)):
        plan = plan_of(case, C.P31)
        assert plan.info()["waves_per_launch"] == 1
        want = same(case, C.P31, plan=plan)
        assert want[0] >= 2 and plan.last_stats["launches"] == 1 + 2 * (-(-case.nb // 64)) >= 5
        p0, p1 = 3, 2 * case.nb - 3
        same(case, C.P31, p0, p1, plan)                                        # the linear launch is not repeated
        wave = lambda pair: (pair // case.nb) * (-(-case.nb // 64)) + (pair % case.nb) // 64
        assert plan.last_stats["launches"] == wave(p1 - 1) - wave(p0) + 1 >= 3
    monkeypatch.delenv("PLO_TPROG_WAVES")
    case = two_far_defects()
    rc, err = C.tool(["--count", "-q", 131071] + case.write(tmp_path), 1, env={"PLO_TPROG_WAVES": "1"})
    want = C.definition(case, 131071)
    assert rc == 1 and C.first_of(err)[0] == want[1] and C.count_of(err)[0] == want[0] and "7 launches" in err


def test_at_the_limit_and_one_above(hip, tmp_path):
    from plinopt_amd import capi
    limit = plan_of(C.schoolbook(1, 2), 131071).info()["max_words"]
    for at, above in C.limit_cases(limit):
        assert at.w == limit and above.w > limit
        assert same(at, C.P31) == (0, None, None, None)
        lines = at.text.splitlines()
        last = max(n for n, ln in enumerate(lines) if " * " in ln)
        bad = at.with_text(at.name + "_bad", "\n".join(lines[:last] + lines[last + 1:]) + "\n")
        assert same(bad, C.P31)[0] >= 1
        with pytest.raises(capi.PloError) as r:
            plan_of(above, C.P31)
        assert r.value.code == -3 and "above the %d state words" % limit in str(r.value)
        dropped = above.with_text(above.name + "_bad", "\n".join(ln for ln in above.text.splitlines() if "a0 * b0" not in ln) + "\n")
        for case in (above, dropped):
            paths = case.write(tmp_path)
            rc0, err0 = C.tool(case.flags() + ["-q", 131071, "--count"] + paths, 0)
            rc1, err1 = C.tool(case.flags() + ["-q", 131071, "--count"] + paths, 1)
            assert rc1 == rc0 == (1 if case is dropped else 0)
            assert "# the device refuses this input (" in err1 and "state words" in err1 and "# host: " in err1 and "# GPU:" not in err1
            assert [ln for ln in tool_lines(err1) if "device refuses" not in ln] == tool_lines(err0)


def fixture_case(name, expanded=False, matmul=False):
    files = [os.path.join(DATA, name + s) for s in ("_L.sms", "_R.sms", "_P.sms")]
    r = subprocess.run([TRILPLACER, "--gpu", "0", "-O", "3"] + (["-e"] if expanded else []) + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return C.Case(name, *(read_sms(f) for f in files), r.stdout, expanded, matmul)


def small_triples():
    import glob
    out = []
    for l in sorted(glob.glob(os.path.join(DATA, "*_L.sms"))):
        r, p = l[:-6] + "_R.sms", l[:-6] + "_P.sms"
        if os.path.exists(r) and os.path.exists(p) and os.path.getsize(l) < 4000:
            try:
                for f in (l, r, p):
                    read_sms(f)
            except ValueError:
                continue
            out.append(os.path.basename(l)[:-6])
    return out


def test_fixture_programs_on_the_device(hip):
    """every program bin/trilplacer prints for the small fixture triples, once, modulo the first certificate prime; -e and -m for a few"""
    names = small_triples()
    assert len(names) >= 10
    for name in names:
        case = fixture_case(name)
        assert device(case, C.P31) == (0, None, None, None), name
    for name in ("1o1o2_3_Karatsuba", "2x2x2_7_Winograd", "4x4x4_48_rational"):
        assert device(fixture_case(name, expanded=True), C.P31) == (0, None, None, None), name
    for name in ("2x2x2_7_Winograd", "3x3x3_23_58", "4x4x4_48_rational"):
        case = fixture_case(name, matmul=True)
        assert same(case, C.P31) == (0, None, None, None), name
        wrong = C.Case(name + "_swapped", case.R, case.L, case.P, case.text)      # B.A instead of A.B
        assert same(wrong, C.P31)[0] >= 1


def test_refusals_of_the_entry_points(hip):
    from plinopt_amd import TProgPlan, capi
    case = C.schoolbook(2, 3)
    L, R, P = case.csr()
    recs = case.records()
    for bad, words in (((3, 0, 0, 0, 0, 0, 1, 1), "unknown family"), ((0, 0, 0, 2, 0, 0, 1, 1), "index out of range"), ((0, 0, 0, 0, 5, 0, 1, 1), "index out of range"),
                       ((2, 2, 0, 0, 0, 0, 2, 1), "coefficient 1 or -1"), ((2, 2, 1, 0, 0, 0, 1, 1), "PLO_TPROG_EXPANDED"), ((0, 1, 0, 0, 0, 0, 1, 0), "non-positive denominator"),
                       ((0, 2, 0, 0, 0, 0, 1, 1), "an AXPY is c[dst]")):
        with pytest.raises(capi.PloError) as r:
            TProgPlan(L, R, P, recs + [bad], 131071)
        assert r.value.code == -1 and words in str(r.value), str(r.value)
    for q in (0, 1, 1 << 31):
        with pytest.raises(capi.PloError) as r:
            TProgPlan(L, R, P, recs, q)
        assert r.value.code == -1 and "modulus" in str(r.value)
    with pytest.raises(capi.PloError) as r:
        TProgPlan(L, R, P, recs, 131071, expanded=True, matmul=True)
    assert r.value.code == -1
    with pytest.raises(capi.PloError) as r:
        TProgPlan(L, R, P, recs, 131071, matmul=True)
    assert r.value.code == -1 and "are not m k, k n and m n" in str(r.value)
    plan = TProgPlan(L, R, P, recs, 131071)
    for p0, p1 in ((0, 0), (3, 2), (0, 7)):
        with pytest.raises(capi.PloError) as r:
            plan.check(p0, p1)
        assert r.value.code == -1 and "pairs" in str(r.value)
