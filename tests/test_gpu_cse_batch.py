"""plo_cse_batch_search (plo_cse_batch.hip: one workgroup per problem, one minimum each) against the C oracle: for every
problem of every batch the cost AND the seed of the minimum over its own seeds seed0 + q*per .. + per-1, and status 0.
PLO_BATCH_GRID=1 makes one workgroup take all problems of a launch in turn (what a longer matrix left in LDS must not be
read by the next one); PLO_WAVE_CAP_TIGHT makes one problem fill its pair table, which only that problem may repeat."""
import pytest

import batch_cases as bc
import synth

pytestmark = pytest.mark.gpu

GRID = "PLO_BATCH_GRID"
INF = (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 64 - 1)


def bucket(foot):
    """the bucket rule of DESIGN.md 2.11: footprints up to 4, 8, 16, 32, 64 KiB and the rest"""
    return next((b for b in range(5) if foot <= 4096 << b), 5)


def foot(plan, second=None):
    return plan.rs_bytes + (second.rs_bytes if second else 0) + max(plan.region_bytes, second.region_bytes if second else 0)


def check(probs, per, seed0=0, mode=0):
    from plinopt_amd import cse_batch_search
    bests, status, st = cse_batch_search([x.csr for x in probs], None, probs[0].p, seed0, per, cost_mode=mode)
    for q, x in enumerate(probs):
        exp = bc.expected(x, seed0 + q * per, per, mode)
        print(q, x.name, bests[q], exp)
        assert status[q] == 0 and bests[q] == exp, (q, x.name)
    return st


@pytest.fixture(scope="module")
def mixed():
    return bc.mixed40()


@pytest.fixture(scope="module")
def chained():
    return bc.chained12()


@pytest.mark.parametrize("per", [1, 2, 3, 5, 7])
def test_one_problem_fewer_candidates_than_waves(hip, per):
    """per_problem below, and no multiple of, the waves of a workgroup: a wave without a candidate must not reach the result"""
    x = bc.from_sms("4x4x4_49_156_L.sms")
    st = check([x], per, seed0=2 ** 40 + 5)
    assert st["launches"] == 1 and st["candidates"] == per and st["grid"] == 1
    assert st["waves_per_wg"] <= max(per, 1) * 2


@pytest.mark.parametrize("grid", [None, "1"])
def test_mixed_batch_of_40(hip, monkeypatch, mixed, grid):
    if grid:
        monkeypatch.setenv(GRID, grid)
    st = check(mixed, 23, seed0=7)
    assert st["candidates"] == 40 * 23
    assert st["launches"] == len({bucket(foot(x.plan)) for x in mixed}) >= 3       # one launch per bucket, nothing repeated
    if grid:
        assert st["grid"] == 1


def test_the_same_matrix_at_three_positions(hip, mixed):
    """Winograd L: most seeds tie, so the winner is each range's smallest seed of the minimal cost"""
    w = bc.from_sms("2x2x2_7_Winograd_L.sms")
    probs = [w, mixed[3], w, mixed[8], mixed[9], w]
    from plinopt_amd import cse_batch_search
    per = 23
    bests, status, _ = cse_batch_search([x.csr for x in probs], None, bc.P, 0, per)
    got = [bests[q] for q in (0, 2, 5)]
    for q, b in zip((0, 2, 5), got):
        assert b == bc.expected(w, q * per, per) and q * per <= b[2] < (q + 1) * per
    assert len({b[:2] for b in got}) == 1 and len({b[2] for b in got}) == 3
    assert status == [0] * 6


@pytest.mark.parametrize("grid", [None, "1"])
def test_chained_problems(hip, monkeypatch, chained, grid):
    from plinopt_amd import cse_batch_search
    if grid:
        monkeypatch.setenv(GRID, grid)
    per, seed0 = 9, 2 ** 33
    bests, status, st = cse_batch_search([a.csr for a, _ in chained], [b.csr for _, b in chained], bc.P, seed0, per)
    for q, (a, b) in enumerate(chained):
        assert status[q] == 0 and bests[q] == bc.expected_chain(a, b, seed0 + q * per, per), (q, a.name)
    assert st["candidates"] == 12 * per
    if grid:
        assert st["grid"] == 1


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_cost_modes(hip, mixed, mode):
    small = [x for x in mixed if not x.plan.unit][:6]
    check(small, 11, seed0=3, mode=mode)


def test_a_refused_problem_between_two_that_fit(hip, mixed):
    from plinopt_amd import capi, cse_batch_search
    bad, code = bc.refused()
    probs, per = [mixed[0], bad, mixed[1]], 5
    bests, status, st = cse_batch_search([x.csr for x in probs], None, bc.P, 0, per)
    assert status == [0, getattr(capi, code), 0] and bests[1] == INF
    for q in (0, 2):
        assert bests[q] == bc.expected(probs[q], q * per, per)
    assert st["candidates"] == 2 * per


def test_only_the_problem_with_a_full_table_is_run_again(hip, monkeypatch, mixed):
    """PLO_WAVE_CAP_TIGHT: tight_general fills its first table (tests/test_gpu_chain_synth.py), the ten quiet problems have
    fewer than 32 triples in the 64 slots every table has at least"""
    O, csr, rows = bc.tight_general()
    tight = bc.from_rows("tight_general", csr[0], csr[1], rows)
    quiet = [x for x in mixed if x.plan.distinct < 32][:10]
    assert len(quiet) == 10
    probs = quiet[:4] + [tight] + quiet[4:]
    per = 6
    monkeypatch.setenv("PLO_WAVE_CAP_TIGHT", "1")
    st = check(probs, per, seed0=11)
    first = len({bucket(foot(synth.wave_plan(x.m, x.n, x.rows, x.p, tight=True))) for x in probs})
    again = st["launches"] - first
    print("launches", st["launches"], "first round", first)
    assert 1 <= again <= 3
    assert st["candidates"] == (len(probs) + again) * per       # every repeat held that one problem
