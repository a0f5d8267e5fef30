"""Inputs of the PLUQ and Householder tests of bin/orbiter (tests/test_orbiter_actions_host.py, tests/test_gpu_orbiter_actions.py,
tests/golden/make_orbit_action_costs.py): small synthetic triples built with the helpers of tests/synth.py, four fixture
triples, the fields, the seeds, and the inputs at the edge of the int64 bound of each action.

Bounds (include/plinopt_hip.h): a part of the sandwich has a direct factor of size sd and an inverse of size si,
(sd, si) = (k, m) for the rows of L, (n, k) for R, (m, n) for the columns of P; the device takes a row over Q when its L1
norm (after scaling to integers) times the product of the two entry bounds stays below 2^62:
  PLUQ         sd x si 4^(si-2)   (1 for si = 1)
  HOUSEHOLDER  sd x si            (numerators over d <= s; the row's scale times sd si must stay below 2^62 too)"""
import random
from fractions import Fraction as F

import synth

TRIANGULAR, PLUQ, HOUSEHOLDER = 0, 1, 2
ACTION_NAMES = {PLUQ: "pluq", HOUSEHOLDER: "householder"}
BASE_SEED = (1 << 64) - 1
SEEDS_LIST = [BASE_SEED] + list(range(16)) + [1 << 63, (1 << 64) - 2]        # scored as one explicit seed list
SEED_RUNS = [(0, 16), (1 << 63, 1), ((1 << 64) - 2, 2)]                      # scored as (seed0, n) runs; the last ends on BASE_SEED
SEEDS_RUNS = [(s0 + j) & BASE_SEED for s0, cnt in SEED_RUNS for j in range(cnt)]
MODULI = [3, 5, 9, 15, 131071, 2147483629]
FIELDS = [(0, synth.DENSITY), (0, synth.CANONICAL)] + [(p, synth.DENSITY) for p in MODULI]
FIXTURES = ["2x2x2_7_Winograd", "2x2x2_7_DPS-accurate", "3x3x3_23_58", "4x4x4_49_156"]
# rationals whose denominators (2, 4, 7) are units of every modulus above: v and -v, v and 1/v, |v| < 1
RATS = [F(2), F(-2), F(1, 2), F(-1, 2), F(7), F(-1, 7), F(2, 7), F(-7, 2), F(3, 4), F(1), F(-1), F(1), F(-3)]
SHAPES = [((1, 1, 1), 1, synth.UNIT), ((2, 2, 2), 7, RATS), ((1, 2, 3), 7, synth.UNIT), ((2, 3, 4), 7, RATS), ((3, 3, 3), 65, synth.UNIT),
          ((3, 9, 2), 7, synth.UNIT), ((2, 16, 3), 1, synth.UNIT), ((1, 2, 3), 65, synth.UNIT)]
TIE_SEED0, TIE_N = synth.TIE_SEED0, synth.TIE_N


def key(action, modulus, measure):
    return "%s|%d|%d" % (ACTION_NAMES[action], modulus, measure)


def mode_of(index):
    return "list" if index % 2 == 0 else "runs"


def seeds_of(mode):
    return list(SEEDS_LIST if mode == "list" else SEEDS_RUNS)


def cases():
    """the synthetic triples (no matrix-multiplication algorithms: the counts are defined for any triple)"""
    rng = random.Random(0xAC7104)
    out = []
    for mkn, r, vals in SHAPES:
        synth._orbit_case(out, "%dx%dx%d_r%d" % (mkn + (r,)), "act", mkn, r, synth._triple(rng, mkn, r, vals))
    return out


def factor_bound(action, sd, si):
    if action == PLUQ:
        return sd * (si * 4 ** (si - 2) if si >= 2 else 1)
    assert action == HOUSEHOLDER
    return sd * si


def bound_cases():
    """per action: a 3x2x4 triple with one row of L, of R and of P^T whose L1 norm times the part's bound is the largest
    value below 2^62 (accepted, in [2^61, 2^62)), and the same triple with the row of P^T at the smallest value that
    reaches 2^62 (PLO_E_UNSUPPORTED).  For Householder also the second bound: a rational row of P^T, +-1/D, whose scale D
    times sd si is the largest value below 2^62, and the smallest that reaches it (its L1 norm after scaling is 2).
    Returns (case, action, refused)."""
    rng = random.Random(0xB0D)
    mkn, r = (3, 2, 4), 3
    m, k, n = mkn
    out, res = [], []
    for action in (PLUQ, HOUSEHOLDER):
        base = synth._triple(rng, mkn, r, synth.UNIT)
        fbs = [factor_bound(action, sd, si) for sd, si in ((k, m), (n, k), (m, n))]
        for refused in (False, True):
            rows = [dict(x) for x in base]
            for part in range(3):
                fb = fbs[part]
                l1 = -((-1 << 62) // fb) if refused and part == 2 else ((1 << 62) - 1) // fb
                assert ((1 << 61) <= l1 * fb < (1 << 62)) != (refused and part == 2) and (l1 - 1) * fb < (1 << 62)
                vals = [l1 - 2 * (l1 // 3), -(l1 // 3), l1 // 3]
                width = (m * k, k * n, m * n)[part]
                rows[part * r + 1] = dict(zip(synth._sample(rng, range(width), 3), [F(v) for v in vals]))
            c = synth._orbit_case(out, "%s_%s" % (ACTION_NAMES[action], "above" if refused else "below"), "bound", mkn, r, rows)
            res.append((c, action, refused))
    base = synth._triple(rng, mkn, r, synth.UNIT)
    fb = factor_bound(HOUSEHOLDER, m, n)
    for refused in (False, True):
        D = -((-1 << 62) // fb) if refused else ((1 << 62) - 1) // fb
        assert ((1 << 61) <= D * fb < (1 << 62)) != refused and 2 * fb < (1 << 62)
        rows = [dict(x) for x in base]
        rows[2 * r + 1] = dict(zip(synth._sample(rng, range(m * n), 2), [F(1, D), F(-1, D)]))
        c = synth._orbit_case(out, "householder_scale_%s" % ("above" if refused else "below"), "bound", mkn, r, rows)
        res.append((c, HOUSEHOLDER, refused))
    return res


def tie_cases():
    """(case, action): the tie-heavy triples of tests/synth.py under PLUQ; for Householder, whose matrices of size 1 and 2 are
    all signed permutations (as are those with d = 1 or 2 at any size: the counts move only when d >= 3), two tiny triples
    with dimensions of 3 and 4, over Q and modulo 5"""
    res = [(c, PLUQ) for c in synth.orbit_tie_cases()]
    rng = random.Random(0x71E3)
    out = []
    synth._orbit_case(out, "3x3x3_Q", "tie3", (3, 3, 3), 3, synth._triple(rng, (3, 3, 3), 3, synth.UNIT, hi=2))
    synth._orbit_case(out, "3x4x3_mod5", "tie3", (3, 4, 3), 3, synth._triple(rng, (3, 4, 3), 3, synth.UNIT, hi=2), modulus=5)
    return res + [(c, HOUSEHOLDER) for c in out]
