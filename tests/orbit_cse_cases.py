"""Inputs and references for the edge-shape tests of the CSE measure of the orbit search (plo_orbit_cse.hip, host side
orbit_cse_layout / orbit_cse_size / plo_orbit_plan_create_cse of plo_capi.hip): no code under test here.

Random sparse triples (synth._triple, synth._orbit_case; values synth.mod_values(p); no matrix-multiplication algorithms: the
measure is defined for any triple), every dimension at most 16, one list per modulus of PRIMES:

  * column bands: the image build gives a row of a part LPR = max(4, 2^ceil_log2(columns)) lanes.  The columns of hP are r
    (shape (2,1,2), r on both sides of every boundary up to 64), those of Lj are mk, those of Rg are kn (32, 33, 63, 64);
  * row-count edges: 64 rows in hP (8,1,8), 64 rows in Lj and Rg (r = 64), one row of 64 columns (1,1,1) with r = 64;
  * dense variants of the 33-, 63- and 64-column cases: one input row of the wide part holds every column with values that
    do not vanish modulo p, so under the base seed (the image is the input) that row of the image has exactly `columns` entries;
  * the refused side of the four limits of the CSE plan (r, mn, mk, kn = 65), each accepted by the density plan.

The references: row lengths and pair instances of a candidate's image from the dense products of tests/orbit_oracle.py, the
table slots the sizing rule of DESIGN 2.9 derives from them, and the costs of tests/orbit_cse_oracle.py, each computed once
per process and shared (tests/test_orbit_cse_cases_host.py checks the properties of these inputs on the CPU)."""
import functools
import random

import orbit_action_oracle as A
import orbit_cse_oracle as Z
import orbit_oracle as O
import synth

BASE = O.BASE_SEED
PRIMES = (131071, 3, 2147483629)
SEEDS = [BASE, 0, 1, 2, 5, 1 << 40]
SUB = 2
LJ, RG, HP = 0, 1, 2
PART = ("Lj", "Rg", "hP")
SIZING_SEEDS = [BASE] + list(range(255))          # the sample of the sizing launch

HP_BANDS = [4, 5, 8, 9, 16, 17, 32, 33, 63, 64]                                    # r of the (2,1,2) cases
LJ_BANDS = [((4, 8, 1), 2), ((3, 11, 1), 3), ((7, 9, 1), 2), ((8, 8, 1), 2)]       # mk = 32, 33, 63, 64
RG_BANDS = [((1, 8, 4), 2), ((1, 11, 3), 3), ((1, 9, 7), 2), ((1, 8, 8), 2)]       # kn = 32, 33, 63, 64
# (shape, r, the quantity above 64, what the refusal says)
REFUSED = [((2, 1, 2), 65, "r", "r or mn above 64"), ((5, 1, 13), 2, "mn", "r or mn above 64"),
           ((5, 13, 1), 2, "mk", "mk or kn above 64"), ((1, 5, 13), 2, "kn", "mk or kn above 64")]


def ceil_log2(x):
    return (x - 1).bit_length()


def dims(c):
    """[(rows, columns)] of the images of Lj, Rg and hP"""
    m, k, n = c.mkn
    return [(c.r, m * k), (c.r, k * n), (m * n, c.r)]


def quantities(c):
    m, k, n = c.mkn
    return {"r": c.r, "mn": m * n, "mk": m * k, "kn": k * n}


def band(cols):
    """log2 of the lanes a row of `cols` columns gets in the image build"""
    return max(2, ceil_log2(cols))


def _nonvanishing(p):
    return [v for v in synth.mod_values(p) if v.numerator % p]


def _densify(rng, rows, mkn, r, part, p):
    """one input row of `part` gets every column: row 0 of L or of R, or row 0 of P (position 0 of every row of P^T)"""
    vals = _nonvanishing(p)
    m, k, n = mkn
    if part == HP:
        for i in range(r):
            rows[2 * r + i][0] = synth._pick(rng, vals)
    else:
        width = m * k if part == LJ else k * n
        rows[part * r] = {j: synth._pick(rng, vals) for j in range(width)}
    return rows


def _case(out, p, name, mkn, r, hi=5, wide=None, dense=False, over=None):
    rng = random.Random("orbit-cse-edges/%s" % name)      # (a string seeds by its sha512: the same on every platform and run)
    rows = synth._triple(rng, mkn, r, synth.mod_values(p), hi=hi)
    if dense:
        rows = _densify(rng, rows, mkn, r, wide, p)
    c = synth._orbit_case(out, name, "cse%d" % p, mkn, r, rows, modulus=p)      # (asserts that the orbit plan's own limits accept it)
    c.wide, c.dense = wide, dense
    c.cols = dims(c)[wide][1] if wide is not None else None
    c.quantity, c.reason = over if over else (None, None)                       # of the refused ones: what is above 64, what the refusal says
    return c


@functools.lru_cache(maxsize=None)
def all_cases(p):
    out = []
    for r in HP_BANDS:
        _case(out, p, "hP_2x1x2_r%d" % r, (2, 1, 2), r, hi=2, wide=HP)
        if r >= 33:
            _case(out, p, "hP_2x1x2_r%d_dense" % r, (2, 1, 2), r, hi=2, wide=HP, dense=True)
    for part, tag, bands in ((LJ, "Lj", LJ_BANDS), (RG, "Rg", RG_BANDS)):
        for mkn, r in bands:
            nm = "%s_%dx%dx%d_r%d" % ((tag,) + mkn + (r,))
            c = _case(out, p, nm, mkn, r, wide=part)
            if c.cols >= 33:
                _case(out, p, nm + "_dense", mkn, r, wide=part, dense=True)
    _case(out, p, "rows_8x1x8_r3", (8, 1, 8), 3)                                  # hP: 64 rows of 3 columns
    _case(out, p, "rows_1x1x1_r64", (1, 1, 1), 64, hi=2, wide=HP)                 # hP: one row of 64 columns; Lj, Rg: 64 rows of one
    _case(out, p, "rows_1x1x1_r64_dense", (1, 1, 1), 64, hi=2, wide=HP, dense=True)
    for mkn, r, q, reason in REFUSED:
        _case(out, p, "over_%s_%dx%dx%d_r%d" % ((q,) + mkn + (r,)), mkn, r, hi=2 if q == "r" else 5, over=(q, reason))
    return out


def accepted(p):
    return [c for c in all_cases(p) if c.quantity is None]


def refused(p):
    return [c for c in all_cases(p) if c.quantity is not None]


def named(p, name):
    """the case `name` (without the family prefix) of modulus p"""
    return next(c for c in all_cases(p) if c.name == "orbit_cse%d_%s" % (p, name))


def wide_cases(p):
    """the accepted cases whose wide part has 33 to 64 columns: the 64-lanes-per-row path"""
    return [c for c in accepted(p) if c.cols is not None and 33 <= c.cols <= 64]


# ---------------------------------------------------------------------------------------------- references
_triples = {}


def triple(c):
    """(qcsr arguments, dense matrices, (m, k, n)) of a case, as tests/test_gpu_orbiter_cse.py::triple"""
    if c.name not in _triples:
        mats = [O.dense(*M) for M in (c.L, c.R, c.P)]
        mats = [M if O.small_ints(M) is None else O.small_ints(M) for M in mats]
        _triples[c.name] = ([synth.qcsr(*M) for M in (c.L, c.R, c.P)], mats, c.mkn)
    return _triples[c.name]


_lengths = {}


def row_lengths(c, seed, action=A.TRIANGULAR):
    """per part the entries of every row of the candidate's image modulo the case's modulus"""
    key = (c.name, seed, action)
    if key not in _lengths:
        _, mats, mkn = triple(c)
        p = c.modulus
        prods = O.products(mats, mkn, seed) if action == A.TRIANGULAR else A.products(mats, mkn, seed, action, p)
        out = []
        for M in prods:
            _, _, rp, _, _ = Z.reduced(M, p)
            out.append([b - a for a, b in zip(rp, rp[1:])])
        _lengths[key] = out
    return _lengths[key]


def pair_instances(lens):
    return sum(l * (l - 1) // 2 for l in lens)


def slots_for(pairs):
    """the first pair table of DESIGN 2.9: the power of two, at least 64, that holds 0.75 x the sampled pair instances + 16"""
    cap = 64
    while cap < pairs * 3 // 4 + 16 and cap < 1 << 17:
        cap <<= 1
    return cap


_slots = {}


def table_slots(c, action=A.TRIANGULAR):
    """(Lj, Rg, hP) slots from the oracle's pair instances, maxima over the sizing sample"""
    key = (c.name, action)
    if key not in _slots:
        worst = [0, 0, 0]
        for s in SIZING_SEEDS:
            for i, lens in enumerate(row_lengths(c, s, action)):
                worst[i] = max(worst[i], pair_instances(lens))
        _slots[key] = tuple(slots_for(x) for x in worst)
    return _slots[key]


_costs = {}


def costs(c, seeds=None, sub=SUB, action=A.TRIANGULAR, cse_seed0=0):
    """[(cost, nnz, nno)] of the literal oracle, computed once per (case, seeds, sub, action)"""
    seeds = SEEDS if seeds is None else seeds
    key = (c.name, tuple(seeds), sub, action, cse_seed0)
    if key not in _costs:
        _, mats, mkn = triple(c)
        _costs[key] = Z.costs(mats, mkn, list(seeds), c.modulus, sub, cse_seed0, action)[0]
    return _costs[key]
