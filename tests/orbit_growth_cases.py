"""Inputs of the growth-factor tests of bin/orbiter -g (tests/test_orbiter_growth_host.py, tests/test_gpu_orbiter_growth.py,
tests/golden/make_orbit_growth_costs.py): fixture triples, small synthetic triples at the edges of plo::orbit_growth_kernel, the
seeds, and the inputs one step inside and one step outside the 2^53 proof of plo_orbit_plan_create_growth.

The proof (include/plinopt_hip.h): for every row g of the 3r rows, with c_g its scale, L1_g its L1 norm after scaling, (sd, si)
the sizes of the part's direct and inverse factor ((k, m) for L, (n, k) for R, (m, n) for P) and B_g = L1_g x the action's
factor bound (triangular 2^(si-2), 1 for si = 1; PLUQ sd x si 4^(si-2), sd for si = 1):  sd si B_g^2 < 2^53 and c_g < 2^53."""
import math
import random
from fractions import Fraction as F

import synth

TRIANGULAR, PLUQ = 0, 1
ACTION_NAMES = {TRIANGULAR: "triangular", PLUQ: "pluq"}
BASE_SEED = (1 << 64) - 1
SEEDS = [BASE_SEED] + list(range(64)) + [1 << 40]         # the GPU tests score all of them
HOST_SEEDS = [BASE_SEED] + list(range(32)) + [1 << 40]    # the host tests: --costs prints the base, then a run
FIXTURES = ["2x2x2_7_Winograd", "2x2x2_7_DPS-integral-12.0662", "3x4x7_63_rational", "4x4x4_49_156"]
HOST_FIXTURES = FIXTURES[:3]
SEARCH_FIXTURES = ["2x2x2_7_Winograd", "4x4x4_49_156"]
SEARCH_N = 4096


def factor_bound(action, sd, si):
    if action == PLUQ:
        return sd * (si * 4 ** (si - 2) if si >= 2 else 1)
    return 1 << max(si - 2, 0)


def growth_refusal(c, action):
    """None when plo_orbit_plan_create_growth takes the case, else the name of its code"""
    base = synth.orbit_refusal(c)                          # the limits of every Q plan (triangular bound, LDS without the sums)
    if base:
        return base
    m, k, n = c.mkn
    nnz = 0
    for g, row in enumerate(synth.orbit_rows(c)):
        lcm = 1
        for _, v in row:
            lcm = lcm * v.denominator // math.gcd(lcm, v.denominator)
        l1 = sum(abs(v * lcm) for _, v in row)
        sd, si = ((k, m), (n, k), (m, n))[g // c.r]
        B = l1 * factor_bound(action, sd, si)
        if B >= 1 << 62 or sd * si * B * B >= 1 << 53 or lcm >= 1 << 53:
            return "PLO_E_UNSUPPORTED"
        nnz += len(row)
    shared, per_wave, _ = synth.orbit_layout(m, k, n, c.r, nnz)
    if action == PLUQ:                                     # the second triangle and its inverse
        smax = max(m, k, n)
        per_wave += synth._ru(8 * smax * smax, 16) + synth._ru(smax * smax, 16)
    per_wave -= synth._ru(2 * 3 * c.r + 2, 16)             # a growth plan keeps no per-row counters
    per_wave = synth._ru(per_wave, 16) + synth._ru(24 * c.r, 16)
    return None if shared + per_wave <= min(synth.LDS_MAX, synth.WG_LDS) else "PLO_E_CAPACITY"


def fixture_case(name):
    """a fixture triple in the form growth_refusal reads.  2x2x2_7_DPS-integral-12.0662 is outside the proof under both actions
    (its rows scale to integers of 31 bits: sd si B^2 is about 2^64.7), so the device refuses it and the host scores it in 128 bits;
    the other three are inside."""
    import os
    from types import SimpleNamespace

    import orbit_oracle as O
    from plo_testlib import DATA, read_sms
    L, R, P = [read_sms(os.path.join(DATA, "%s_%s.sms" % (name, x))) for x in "LRP"]
    return SimpleNamespace(name=name, mkn=O.shape(L[:2], R[:2], P[:2]), r=L[0], L=L, R=R, P=P, modulus=0)


def cases():
    """the synthetic triples (no matrix-multiplication algorithms: the measure is defined for any triple):
    r = 1 with m = k = n = 1; (1, 2, 3); r = 63, 64, 65 (the lane stride of the term loop and of the sums); an L row, an R row and
    a column of P without entries (terms 0); a dimension of 16 with r = 2 (PLUQ: outside the proof); rows with different denominators"""
    rng = random.Random(0x6F0)
    out = []
    synth._orbit_case(out, "1x1x1_r1", "growth", (1, 1, 1), 1, synth._triple(rng, (1, 1, 1), 1, synth.RATS))
    synth._orbit_case(out, "1x2x3_r7", "growth", (1, 2, 3), 7, synth._triple(rng, (1, 2, 3), 7, synth.UNIT))
    for r in (63, 64, 65):
        synth._orbit_case(out, "2x2x2_r%d" % r, "growth", (2, 2, 2), r, synth._triple(rng, (2, 2, 2), r, synth.RATS))
    rows = synth._triple(rng, (2, 3, 2), 5, synth.RATS)
    rows[1], rows[5 + 3], rows[10 + 4] = {}, {}, {}
    synth._orbit_case(out, "2x3x2_empty_rows", "growth", (2, 3, 2), 5, rows)
    synth._orbit_case(out, "16x2x3_r2", "growth", (16, 2, 3), 2, synth._triple(rng, (16, 2, 3), 2, synth.UNIT))
    synth._orbit_case(out, "2x3x4_rats", "growth", (2, 3, 4), 7, synth._triple(rng, (2, 3, 4), 7, synth.RATS))
    return out


def bound_cases():
    """per action: a 3x2x4 triple with a row of P^T (sd si = 12 outputs) whose L1 norm makes 12 B^2 the largest value below
    2^53 (accepted), and the same triple with that row one larger (12 B^2 >= 2^53: PLO_E_UNSUPPORTED).
    Returns (case, action, refused)."""
    rng = random.Random(0x253)
    mkn, r = (3, 2, 4), 3
    m, k, n = mkn
    out, res = [], []
    for action in (TRIANGULAR, PLUQ):
        base = synth._triple(rng, mkn, r, synth.UNIT)
        fb = factor_bound(action, m, n)
        l1 = math.isqrt(((1 << 53) - 1) // (m * n)) // fb
        assert m * n * (l1 * fb) ** 2 < (1 << 53) <= m * n * ((l1 + 1) * fb) ** 2
        cols = synth._sample(rng, range(m * n), 3)
        for refused in (False, True):
            x = l1 + 1 if refused else l1
            rows = [dict(d) for d in base]
            rows[2 * r + 1] = dict(zip(cols, [F(x - 2 * (x // 3)), F(-(x // 3)), F(x // 3)]))
            c = synth._orbit_case(out, "%s_%s" % (ACTION_NAMES[action], "outside" if refused else "inside"), "growth_bound", mkn, r, rows)
            assert (growth_refusal(c, action) == "PLO_E_UNSUPPORTED") == refused and growth_refusal(c, action) in (None, "PLO_E_UNSUPPORTED")
            res.append((c, action, refused))
    return res
