"""Seeded synthetic matrices over Z_p for the parity sweeps (SURVEY.md 8d "synthetic inputs")."""
import hashlib
import math
import random
from fractions import Fraction as F
from types import SimpleNamespace


def small_valued(seed, p, mmax=7, nmax=6, density=0.6):
    """Small matrices with coefficients from a tiny set: provokes repeated
    coefficients per column/row and <ab|b;a|.> triangles (ProgramGen paths)."""
    rng = random.Random(seed)
    m, n = rng.randint(2, mmax), rng.randint(2, nmax)
    vals = [1, -1, 2, -2, 3, 4, 6, -6, 12, pow(2, -1, p), pow(3, -1, p)]
    rows = []
    for _ in range(m):
        r = {}
        for j in range(n):
            if rng.random() < density:
                r[j] = rng.choice(vals) % p
        rows.append(r)
    return m, n, rows


def sweep(seed, p, m, n, density=0.25, unit_frac=0.8):
    """row density 25 %, values from {1,-1} (80 %) and {2,-2,1/2,-1/2} (20 %)."""
    rng = random.Random(seed)
    h = pow(2, -1, p)
    rows = []
    for _ in range(m):
        r = {}
        for j in range(n):
            if rng.random() < density:
                r[j] = (rng.choice([1, p - 1]) if rng.random() < unit_frac else rng.choice([2, p - 2, h, p - h]))
        rows.append(r)
    return m, n, rows


def to_csr(rows, p):
    rp, c, v = [0], [], []
    for r in rows:
        for j, x in sorted(r.items()):
            if x % p:
                c.append(j)
                v.append(x % p)
        rp.append(len(c))
    return rp, c, v


# ======================================================================================================================
# Edge-shape cases for the in-place linear kernel (plo_lin.hip, bin/inplacer) and the orbit kernel (plo_orbit.hip,
# bin/orbiter): pure Python, exact Fractions, one fixed seed, no input file.  tests/golden/make_lin_synth_costs.py and
# make_orbit_synth_costs.py score them with the literal oracles; tests/test_gpu_lin_orbit_synth.py holds the kernels and
# tests/test_synth_golden.py the host engines to those goldens.
#
# Every accepted case is checked HERE, by the arithmetic of the documented limits (include/plinopt_hip.h and the byte
# layouts of plo_lin_plan_create_q / plo_orbit_plan_create_q), to be one the device takes: a case that drifts over a limit
# fails on the CPU, and the GPU tests assert that nothing but the named refusal cases is refused.
# ======================================================================================================================
BASE_SEED = (1 << 64) - 1
BIG_SEEDS = [1 << 63, (1 << 64) - 2]
SEEDS_LIST = [BASE_SEED] + list(range(8)) + BIG_SEEDS            # scored as one explicit seed list
SEED_RUNS = [(0, 8), (1 << 63, 1), ((1 << 64) - 2, 2)]           # scored as (seed0, n) runs; the last one ends on BASE_SEED
SEEDS_RUNS = [s0 + j for s0, cnt in SEED_RUNS for j in range(cnt)]
TIE_SEED0, TIE_N = 5, 2000                                       # the tie-heavy searches: seeds 5 .. 2004

DENSITY, CANONICAL = 0, 2
LIN_PRIME = 2147483629                                           # residues of the rational device programs
LDS_MAX, WG_LDS = 160 * 1024, 64 * 1024
UNIT = [F(1), F(-1)]
# v and -v, v and 1/v, |v| < 1, each several times: cumulations cancel (isnoop) or give +-1 (no SCA)
RATS = [F(2), F(-2), F(1, 2), F(-1, 2), F(3), F(-3), F(1, 3), F(-1, 3), F(2, 3), F(-2, 3), F(3, 2), F(1), F(-1), F(1), F(2)]


def _ru(x, a):
    return (x + a - 1) // a * a


def _pick(rng, seq):
    return seq[rng.randrange(len(seq))]


def _sample(rng, pool, k):
    """k distinct elements of pool, by a partial Fisher-Yates on randrange alone"""
    pool = list(pool)
    assert k <= len(pool)
    for i in range(k):
        j = i + rng.randrange(len(pool) - i)
        pool[i], pool[j] = pool[j], pool[i]
    return pool[:k]


def fstr(v):
    return str(v.numerator) if v.denominator == 1 else "%d/%d" % (v.numerator, v.denominator)


def sms_text(m, n, ent):
    """the matrix as the tools read it (1-based, rational)"""
    return "%d %d R\n" % (m, n) + "".join("%d %d %s\n" % (i + 1, j + 1, fstr(v)) for (i, j), v in sorted(ent.items())) + "0 0 0\n"


def qcsr(m, n, ent):
    """(m, n, rowptr, col, num, den) of plo_qcsr_t"""
    rp, col, num, den = [0], [], [], []
    byrow = [[] for _ in range(m)]
    for (i, j), v in sorted(ent.items()):
        byrow[i].append((j, v))
    for row in byrow:
        for j, v in row:
            col.append(j); num.append(v.numerator); den.append(v.denominator)
        rp.append(len(col))
    return m, n, rp, col, num, den


def _sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


# ---------------------------------------------------------------------------------------------------- in-place linear
def lin_layout(m, nnz):
    """(cap, lds_per_wave, waves per workgroup, LDS bytes of a workgroup) as plo_lin_plan_create_q sizes them"""
    cap = _ru(4 * nnz + 3 * m + 2, 64)
    per_wave = _ru(8 * cap + 2 * ((m + 1) & ~1), 16)
    waves = 4 if 4 * per_wave <= WG_LDS else 1
    return cap, per_wave, waves, waves * per_wave


def lin_refusal(m, n, ent):
    """None when the device takes the matrix, else the name of the header's code (include/plinopt_hip.h, plo_lin_*)"""
    if m > 16382 or n > 16382:
        return "PLO_E_CAPACITY"
    lens = [0] * m
    for (i, _), v in ent.items():
        lens[i] += 1
        assert v != 0 and abs(v.numerator) < (1 << 63) and v.denominator < (1 << 63)
        if v.numerator % LIN_PRIME == 0 or v.denominator % LIN_PRIME == 0:
            return "PLO_E_UNSUPPORTED"
    if max(lens) > 64:
        return "PLO_E_UNSUPPORTED"
    cap, _, _, lds = lin_layout(m, len(ent))
    if cap > 65535 or lds > LDS_MAX:
        return "PLO_E_CAPACITY"
    return None


def lin_quick(m, nnz, unit):
    """The cases whose goldens tests/test_synth_golden.py recomputes: those the literal oracle scores in under a second
    (tests/golden/make_lin_synth_costs.py prints the times).  A fixed rule on the size and not the measured time, so that
    the JSON is reproduced byte for byte: the oracle's time grows with the program's length 4 nnz + 3 m, and is about
    twice as long over the rationals.  Rows of 63 and 64 entries (family c) do not follow it and say which they are."""
    return (4 * nnz + 3 * m) * (1 if unit else 2) <= 1750


def _lin_case(out, name, family, m, n, rows, refusal=None, quick=None):
    """rows: one {column: value} per row"""
    assert len(rows) == m and all(0 <= j < n for r in rows for j in r)
    ent = {(i, j): F(v) for i, r in enumerate(rows) for j, v in r.items()}
    assert lin_refusal(m, n, ent) == refusal, (name, lin_refusal(m, n, ent))
    by_list = len(out) % 2 == 0                       # half as an explicit seed list, half as (seed0, n) runs
    nnz, unit = len(ent), all(v in (1, -1) for v in ent.values())
    c = SimpleNamespace(name="lin_%s_%s" % (family, name), family=family, m=m, n=n, ent=ent, nnz=nnz, refusal=refusal,
                        mode="list" if by_list else "runs", seeds=list(SEEDS_LIST if by_list else SEEDS_RUNS),
                        unit=unit, waves=lin_layout(m, nnz)[2],
                        quick=lin_quick(m, nnz, unit) if quick is None else quick)
    c.sha256 = _sha(sms_text(m, n, ent))
    assert c.name not in [x.name for x in out], c.name
    out.append(c)
    return c


def _rows(rng, n, lens, vals, pool=None):
    pool = list(range(n)) if pool is None else pool
    return [{j: _pick(rng, vals) for j in _sample(rng, pool, ln)} for ln in lens]


def lin_cases():
    """About 60 matrices at the edges of lin_kernel / t_linear<LIN_X> / t_simplify, and two the device refuses."""
    rng = random.Random(0x11A5E5)
    out = []
    flavours = (("unit", UNIT), ("rat", RATS))
    # (a) row-count edges: the strided permutation fill (k += 64) and m around one and two waves' worth of rows
    for m in (1, 2, 63, 64, 65, 128, 129):
        for fl, vals in flavours:
            n = 7
            _lin_case(out, "m%d_%s" % (m, fl), "a", m, n, _rows(rng, n, [1 + rng.randrange(4) for _ in range(m)], vals))
    # (b) empty rows (TL_EMPTYBAR): 5-50 %, first row, last row, two in a row
    for m, empty in [(20, [0]), (20, [19]), (20, [7, 8]), (20, [0, 1, 18, 19]), (24, [0, 5, 6, 11, 12, 13, 17, 20, 21, 22, 23, 3]),
                     (40, [9, 30]), (9, [1, 2, 3, 4])]:
        for fl, vals in flavours:
            n = 6
            rows = _rows(rng, n, [0 if i in empty else 1 + rng.randrange(4) for i in range(m)], vals)
            assert 0.05 <= len(empty) / m <= 0.5
            _lin_case(out, "%dof%d_%s_%s" % (len(empty), m, "-".join(map(str, empty[:4])), fl), "b", m, n, rows)
    # (c) long rows: lengths 1, 2, 63 and 64 (a full wave in the ballots of t_linear), at most 6 long rows, under 400 entries
    # (quick: under a second of oracle time; three or more long unit rows take the oracle 20 s, two among short rows 1.5 s)
    for name, n, lens, vals, quick in [("full_unit", 64, [64, 1, 63, 2], UNIT, True), ("four_unit", 70, [64, 64, 63, 63, 2, 1], UNIT, False),
                                       ("full_rat", 64, [64, 63, 1, 2, 5], RATS, True), ("wide_rat", 100, [63, 64, 2, 1, 64], RATS, True),
                                       ("ones", 64, [64, 64, 63], [F(1)], False), ("mixed_unit", 66, [1, 2, 63, 64, 3, 4, 5, 3, 4, 5], UNIT, False),
                                       ("minus_rat", 64, [64, 64], [F(-1), F(-1), F(2)], True)]:
        assert sum(ln >= 63 for ln in lens) <= 6 and sum(lens) < 400
        _lin_case(out, name, "c", len(lens), n, _rows(rng, n, lens, vals), quick=quick)
    # (d) high columns: the 14-bit src/des fields next to the "none" code 0x3FFF; columns n-1 and n-2 as pivots
    # (single-entry rows, and every entry of a row may be drawn as the pivot) and as operands
    for n in (16382, 8193, 300):
        for fl, vals in flavours:
            pool = [0, 1, n // 2, n - 3, n - 2, n - 1]
            rows = [{n - 1: vals[0]}, {n - 2: vals[1]}, {n - 1: vals[1], n - 2: vals[0]}, {0: vals[0], n - 1: vals[0]}, {n - 2: vals[0], 1: vals[1]}]
            rows += _rows(rng, n, [2 + rng.randrange(3) for _ in range(9)], vals, pool)
            _lin_case(out, "n%d_%s" % (n, fl), "d", len(rows), n, rows)
    # (e) duplicated and negated rows over 4-6 columns: as many merges and no-ops as the simplification can meet
    for n in (4, 5, 6):
        for fl, vals in flavours:
            basis = _rows(rng, n, [2 + rng.randrange(n - 2) for _ in range(3)], vals)
            rows = []
            for _ in range(14 + n):
                r = dict(_pick(rng, basis))
                rows.append({j: -v for j, v in r.items()} if rng.randrange(3) == 0 else r)
            _lin_case(out, "n%d_%s" % (n, fl), "e", len(rows), n, rows)
    # (f) single-entry rows: no addition at all, the scaling atoms alone (1: nothing, -1 and others: * and /)
    for name, vals in [("ones", [F(1)]), ("signs", UNIT), ("rat", RATS), ("minus", [F(-1)]), ("halves", [F(1, 2), F(2), F(-1, 2)])]:
        _lin_case(out, name, "f", 12, 5, _rows(rng, 5, [1] * 12, vals))
    _lin_case(out, "among_rat", "f", 12, 5, _rows(rng, 5, [1, 3, 1, 1, 2, 1, 4, 1, 1, 2, 1, 1], RATS))
    # (g) one wave per workgroup: 4 * lds_per_wave passes 64 KiB
    for fl, vals, m, n in (("unit", UNIT, 220, 40), ("rat", RATS, 180, 30)):
        c = _lin_case(out, fl, "g", m, n, _rows(rng, n, [1 + rng.randrange(4) for _ in range(m)], vals))
        assert not c.quick and 2046 < 4 * c.nnz + 3 * m <= 4000 and c.waves == 1
    # (h) near the 160 KiB of LDS: few columns, so that the walks of the simplification stay short for the oracle
    m, n = 1500, 6
    c = _lin_case(out, "unit", "h", m, n, _rows(rng, n, [1 + rng.randrange(3) for _ in range(m)], UNIT))
    assert not c.quick and 16000 <= 4 * c.nnz + 3 * m <= 20000 and c.waves == 1 and lin_layout(m, c.nnz)[3] > 128 * 1024
    # (i) walks longer than the lock-step prefix of t_simplify (PLO_TRIL_LOCKSTEPS): 200 rows of 2 entries over 400 columns
    for fl, vals in flavours:
        _lin_case(out, fl, "i", 200, 400, _rows(rng, 400, [2] * 200, vals))
    assert all(c.waves == 4 for c in out if c.family in "abcdef")
    # refusals: a row of 65 entries, and one row more than an atom's 14-bit variables hold
    _lin_case(out, "row65", "refuse", 3, 70, _rows(rng, 70, [65, 2, 3], UNIT), refusal="PLO_E_UNSUPPORTED", quick=False)
    _lin_case(out, "m16383", "refuse", 16383, 5, _rows(rng, 5, [2 if i % 4096 == 7 else 0 for i in range(16383)], UNIT), refusal="PLO_E_CAPACITY", quick=False)
    return out


def lin_tie_cases():
    """three tiny matrices whose candidates tie all the time: the argmin under (ADD, SCA, seed, variant)"""
    rng = random.Random(0x71E5)
    out = []
    _lin_case(out, "3x3", "tie", 3, 3, _rows(rng, 3, [3, 3, 3], UNIT))
    _lin_case(out, "2x3", "tie", 2, 3, _rows(rng, 3, [2, 3], UNIT))
    _lin_case(out, "4x3_empty", "tie", 4, 3, _rows(rng, 3, [2, 0, 3, 2], RATS))
    return out


# ---------------------------------------------------------------------------------------------------- orbit
def orbit_rows(c):
    """the rows of L, of R and of P^T (what the kernel transforms), each a sorted list of (column, value)"""
    r = c.r
    rows = [[] for _ in range(3 * r)]
    for (i, j), v in sorted(c.L[2].items()):
        rows[i].append((j, v))
    for (i, j), v in sorted(c.R[2].items()):
        rows[r + i].append((j, v))
    for (i, j), v in sorted(c.P[2].items()):
        rows[2 * r + j].append((i, v))
    return rows


def orbit_layout(m, k, n, r, nnz):
    """(shared bytes, bytes per wave, waves per workgroup) as plo_orbit_plan_create_q sizes them; waves 0: does not fit"""
    nrows, smax = 3 * r, max(m, k, n)
    shared = _ru(8 * nnz, 16) + _ru(8 * nrows, 16) + _ru(4 * (nrows + 1), 16) + _ru(2 * nnz, 16)
    per_wave = sum(_ru(8 * s * s, 16) for s in (m, k, k, n, m, n)) + _ru(8 * smax * smax, 16) + _ru(smax * smax, 16) + 32 + _ru(2 * nrows + 2, 16)
    for w in (4, 2, 1):
        if shared + w * per_wave <= min(LDS_MAX, WG_LDS):
            return shared, per_wave, w
    return shared, per_wave, 0


def orbit_refusal(c):
    """None when the device takes the case, else the name of the header's code (include/plinopt_hip.h, plo_orbit_*);
    sets c.waves and c.dev_nnz (the entries left after those that vanish modulo the modulus are dropped)"""
    m, k, n = c.mkn
    p = c.modulus
    if p >= 1 << 31:
        return "PLO_E_UNSUPPORTED"
    if max(m, k, n) > 16 or c.r > 4096 or c.r * (m * k + k * n + m * n) >= 1 << 21:
        return "PLO_E_CAPACITY"
    nnz = 0
    for g, row in enumerate(orbit_rows(c)):
        if p:
            for _, v in row:
                if math.gcd(v.denominator, p) != 1:
                    return "PLO_E_UNSUPPORTED"
                nnz += v.numerator % p != 0
        else:
            lcm = 1
            for _, v in row:
                lcm = lcm * v.denominator // math.gcd(lcm, v.denominator)
            l1 = sum(abs(v * lcm) for _, v in row)
            s = (m, k, n)[g // c.r]
            if lcm > 1 << 62 or l1 * (1 << max(s - 2, 0)) >= 1 << 62:
                return "PLO_E_UNSUPPORTED"
            nnz += len(row)
    c.dev_nnz = nnz
    c.waves = orbit_layout(m, k, n, c.r, nnz)[2]
    return None if c.waves else "PLO_E_CAPACITY"


def orbit_text(c):
    return "%d %d\n" % (c.modulus, c.measure) + "".join(sms_text(*M) for M in (c.L, c.R, c.P))


def orbit_quick(m, k, n, modulus):
    """The cases whose goldens tests/test_synth_golden.py recomputes: those the literal oracle scores in under a second
    (tests/golden/make_orbit_synth_costs.py prints the times).  A fixed rule on the size and not the measured time, so that
    the JSON is reproduced byte for byte: the oracle's time follows the squares of the three Kronecker factors' sizes, r
    hardly matters, and it is about twice as long under a modulus."""
    return ((m * k) ** 2 + (k * n) ** 2 + (m * n) ** 2) * (2 if modulus else 1) <= 25000


def _orbit_case(out, name, family, mkn, r, rows, modulus=0, measure=DENSITY, refusal=None, quick=None):
    """rows: 3r dicts {position: value}: the rows of L (r x mk), of R (r x kn) and of P^T (r x mn)"""
    m, k, n = mkn
    assert len(rows) == 3 * r
    L = (r, m * k, {(i, j): F(v) for i in range(r) for j, v in rows[i].items()})
    R = (r, k * n, {(i, j): F(v) for i in range(r) for j, v in rows[r + i].items()})
    P = (m * n, r, {(j, i): F(v) for i in range(r) for j, v in rows[2 * r + i].items()})
    by_list = len(out) % 2 == 0
    c = SimpleNamespace(name="orbit_%s_%s" % (family, name), family=family, mkn=tuple(mkn), r=r, L=L, R=R, P=P, modulus=modulus, measure=measure,
                        refusal=refusal, mode="list" if by_list else "runs", seeds=list(SEEDS_LIST if by_list else SEEDS_RUNS), waves=None, dev_nnz=None)
    assert all(v != 0 and abs(v.numerator) < (1 << 63) and v.denominator < (1 << 63) for M in (L, R, P) for v in M[2].values())
    got = orbit_refusal(c)
    assert got == refusal, (c.name, got)
    c.nnz = len(L[2]) + len(R[2]) + len(P[2])
    c.quick = orbit_quick(m, k, n, modulus) if quick is None else quick
    c.sha256 = _sha(orbit_text(c))
    assert c.name not in [x.name for x in out], c.name
    out.append(c)
    return c


def _triple(rng, mkn, r, vals, hi=5):
    m, k, n = mkn
    rows = []
    for width in (m * k, k * n, m * n):
        rows += _rows(rng, width, [1 + rng.randrange(min(hi, width)) for _ in range(r)], vals)
    return rows


def _vanishing(rng, rows, p, den=1):
    """one entry of the triple becomes a multiple of p: it vanishes modulo p and the host drops it"""
    g = rng.randrange(len(rows))
    j = sorted(rows[g])[0]
    rows[g][j] = F(p * (1 + rng.randrange(2)), den)
    return rows


def mod_values(p):
    """+-1 mostly, small integers, and rationals whose denominators are units modulo p"""
    dens = [d for d in (2, 3, 5, 7) if p % d][:2]
    assert len(dens) == 2
    return [F(1), F(-1), F(1), F(-1), F(2), F(-3), F(1, dens[0]), F(-1, dens[0]), F(dens[0], dens[1]), F(-2, dens[1])]


A_SHAPES = [((1, 1, 1), 2), ((16, 1, 1), 1), ((1, 16, 9), 33), ((8, 8, 8), 64), ((9, 9, 9), 65), ((16, 16, 16), 33), ((11, 12, 13), 2), ((8, 13, 16), 64)]


def orbit_cases():
    """About 50 random sparse triples (r x mk, r x kn, mn x r; no matrix-multiplication algorithms: the counts are defined
    for any triple) at the edges of orbit_kernel / o_zoi, and three the device refuses."""
    rng = random.Random(0x0B17)
    out = []
    # (a) dimension edges (s*s > 64: more than one trip of the strided loops of o_zoi; 16: full P/Q halves and |T^-1| up to
    # 2^14; 1: no Fisher-Yates draw) with r in {1, 2, 33, 64, 65}; (e) the same triples under the canonical measure
    for mkn, r in A_SHAPES + [((1, 1, 1), 65), ((16, 16, 16), 1), ((16, 16, 16), 65)]:
        rows = _triple(rng, mkn, r, UNIT)
        nm = "%dx%dx%d_r%d" % (mkn + (r,))
        _orbit_case(out, nm, "a", mkn, r, rows)
        if (mkn, r) in A_SHAPES:
            _orbit_case(out, nm, "e", mkn, r, rows, measure=CANONICAL)
    # (b) workgroup paths: 4, 2 and 1 waves per workgroup by the byte layout; 3r odd and even under -c (the packed 16-bit counters)
    for name, mkn, r, ms, waves in [("waves4", (16, 16, 16), 20, DENSITY, 4), ("waves2", (16, 16, 16), 70, DENSITY, 2), ("waves1", (16, 16, 16), 300, DENSITY, 1),
                                    ("canon_3r_odd", (3, 4, 5), 35, CANONICAL, 4), ("canon_3r_even", (3, 4, 5), 36, CANONICAL, 4),
                                    ("canon_waves1", (16, 16, 16), 301, CANONICAL, 1)]:
        c = _orbit_case(out, name, "b", mkn, r, _triple(rng, mkn, r, UNIT), measure=ms)
        assert c.waves == waves, (name, c.waves)
    # (c) fields: Q with +-1, Q with rationals, prime and composite moduli up to 2^31 - 1; under a modulus one entry vanishes
    _orbit_case(out, "Q_unit", "c", (3, 4, 5), 12, _triple(rng, (3, 4, 5), 12, UNIT))
    _orbit_case(out, "Q_rat", "c", (3, 4, 5), 12, _triple(rng, (3, 4, 5), 12, RATS))
    _orbit_case(out, "Q_rat_canon", "c", (4, 3, 2), 9, _triple(rng, (4, 3, 2), 9, RATS), measure=CANONICAL)
    _orbit_case(out, "Q_rat_16", "c", (16, 16, 16), 6, _triple(rng, (16, 16, 16), 6, RATS))
    for p in (3, 5, 9, 15, 131071, 2147483629, 2147483647, 2147483645):
        mkn = _pick(rng, [(2, 3, 4), (3, 3, 3), (4, 2, 3), (2, 2, 5)])
        rows = _vanishing(rng, _triple(rng, mkn, 10, mod_values(p)), p, den=_pick(rng, [1, mod_values(p)[6].denominator]))
        c = _orbit_case(out, "mod%d" % p, "c", mkn, 10, rows, modulus=p)
        assert c.dev_nnz < c.nnz
    for p, mkn, r in ((3, (16, 16, 16), 8), (2147483647, (9, 9, 9), 8), (15, (10, 16, 9), 8), (2147483645, (16, 9, 10), 8)):
        rows = _vanishing(rng, _triple(rng, mkn, r, mod_values(p)), p)
        c = _orbit_case(out, "mod%d_%dx%dx%d" % ((p,) + mkn), "c", mkn, r, rows, modulus=p)
        assert c.dev_nnz < c.nnz
    # (d) over Q just under the bound of exact counts: dimension 16, one row each of L, R and P^T with L1 * 2^14 in [2^61, 2^62)
    for name, big in (("low", [(1 << 45) + 1, -((1 << 45) + 3), (1 << 45) + 5, (1 << 46) + 7]), ("high", [(1 << 47) - 1, -(1 << 46), 1 << 45, (1 << 45) - 1])):
        mkn, r = (16, 16, 16), 3
        rows = _triple(rng, mkn, r, UNIT)
        for part in range(3):
            g = part * r + rng.randrange(r)
            rows[g] = dict(zip(_sample(rng, range(256), len(big)), [F(x) for x in big]))
            assert (1 << 61) <= sum(abs(x) for x in big) << 14 < (1 << 62)
        _orbit_case(out, name, "d", mkn, r, rows)
    # (f) the canonical measure asked for under a modulus: scored by density, as the header, the tool and the oracle do
    for mkn, r in (((3, 4, 5), 12), ((9, 2, 3), 7)):
        rows = _vanishing(rng, _triple(rng, mkn, r, mod_values(131071)), 131071)
        _orbit_case(out, "%dx%dx%d" % mkn, "f", mkn, r, rows, modulus=131071, measure=CANONICAL)
    # refusals: a dimension of 17, a modulus of 2^31, a denominator that is no unit of the modulus
    _orbit_case(out, "dim17", "refuse", (17, 1, 2), 4, _triple(rng, (17, 1, 2), 4, UNIT), refusal="PLO_E_CAPACITY", quick=False)
    _orbit_case(out, "mod2p31", "refuse", (2, 2, 2), 4, _triple(rng, (2, 2, 2), 4, UNIT), modulus=1 << 31, refusal="PLO_E_UNSUPPORTED", quick=False)
    rows = _triple(rng, (2, 2, 2), 4, UNIT)
    rows[5][sorted(rows[5])[0]] = F(1, 3)
    _orbit_case(out, "den3_mod9", "refuse", (2, 2, 2), 4, rows, modulus=9, refusal="PLO_E_UNSUPPORTED", quick=False)
    return out


def orbit_tie_cases():
    """three tiny triples whose candidates tie all the time: the argmin under (cost, nnz, nno, seed)"""
    rng = random.Random(0x71E6)
    out = []
    _orbit_case(out, "2x2x2_mod3", "tie", (2, 2, 2), 3, _triple(rng, (2, 2, 2), 3, UNIT, hi=2), modulus=3)
    _orbit_case(out, "1x2x2_Q", "tie", (1, 2, 2), 3, _triple(rng, (1, 2, 2), 3, UNIT, hi=2))
    _orbit_case(out, "2x1x2_Q_canon", "tie", (2, 1, 2), 4, _triple(rng, (2, 1, 2), 4, UNIT, hi=2), measure=CANONICAL)
    return out


# ======================================================================================================================
# Edge-shape cases for the kernel method (plo_kmethod.hip, plo_kernel_search) and the trilinear kernel (plo_tril.hip,
# plo_tril_*): tests/golden/make_kmethod_synth_costs.py and make_tril_synth_costs.py score them with the C oracle
# (oracle/plo_oracle.c plo_oracle_kernel_restart, oracle/plo_tril_oracle.c); tests/test_gpu_kmethod_tril_synth.py holds the
# kernels to those goldens and tests/test_synth_golden.py recomputes them.
# ======================================================================================================================
KM_PRIME = 131071
KM_MODULI = [3, 5, 7, 101, 8191, 524287, 2147483629, 2147483647]
KM_R = [4, 5, 8, 9, 16, 17, 32, 33, 64]
KM_PER_BLOCK = (1000, 50, 16)                                    # seed0, restarts and per_block of the shared-decomposition check


def _clog2(x):
    return max(x - 1, 0).bit_length()


def rank_mod(rows, p):
    """rank modulo p of rows given as {column: value}"""
    piv, r = {}, 0
    for row in rows:
        row = {j: v % p for j, v in row.items() if v % p}
        while row:
            j = min(row)
            if j not in piv:
                iv = pow(row[j], -1, p)
                piv[j] = {k: v * iv % p for k, v in row.items()}
                r += 1
                break
            x = row[j]
            for k, v in piv[j].items():
                w = (row.get(k, 0) - x * v) % p
                if w:
                    row[k] = w
                else:
                    row.pop(k, None)
    return r


def km_refusal(m, n, rows, p):
    """None when plo_kernel_search takes the matrix as far as the host can tell without a device (Dep's pair table is sized
    from a sample of the decompositions on the device: a dense Dep is refused for capacity there), else the name of the
    header's code, in the order plo_kernel_search checks"""
    if m == 0 or m > 128 or n == 0 or n > 64:
        return "PLO_E_UNSUPPORTED"
    R = rank_mod(rows, p)
    nd = m - R
    if nd == 0 or nd > 64 or R == 0:
        return "PLO_E_UNSUPPORTED"
    unit = all(v % p in (1, p - 1) for r in rows for v in r.values())
    if m > 64 and not unit:
        return "PLO_E_CAPACITY"
    naive = sum(max(len(r) - 1, 0) for r in rows)
    for cols, nv in ((n, naive), (m, nd * R)):                   # the pair keys of M's image and, at its hard bound, of Dep's
        nc = cols + nv // 2 + 2
        if nc >= 0xFFFF or 2 * _clog2(nc) + _clog2(p) > 51:
            return "PLO_E_CAPACITY"
    if 2 * sum(len(r) for r in rows) >= 65535 or 2 * nd * R >= 65535:
        return "PLO_E_CAPACITY"
    return None


def km_text(m, n, p, rows):
    return "%d %d %d\n" % (m, n, p) + "".join("%d %d %d\n" % (i, j, v) for i, r in enumerate(rows) for j, v in sorted(r.items()))


def _km_case(out, name, family, n, rows, p=KM_PRIME, refusal=None):
    """rows: one {column: signed value} per row; the case holds the residues"""
    m = len(rows)
    assert all(0 <= j < n and v % p for r in rows for j, v in r.items()), name
    rows = [{j: v % p for j, v in r.items()} for r in rows]
    got = km_refusal(m, n, rows, p)
    assert got == refusal, (name, got)
    unit = all(v in (1, p - 1) for r in rows for v in r.values())
    assert m <= 64 or unit or refusal, name                      # more than 64 rows: +-1 only
    rank = rank_mod(rows, p) if n <= 64 and m <= 128 else None
    c = SimpleNamespace(name="km_%s_%s" % (family, name), family=family, m=m, n=n, p=p, rows=rows, csr=(m, n) + to_csr(rows, p), refusal=refusal,
                        mode="runs", seeds=list(SEEDS_RUNS), unit=unit, rank=rank, quick=not refusal, sha256=_sha(km_text(m, n, p, rows)))
    assert c.name not in [x.name for x in out], c.name
    out.append(c)
    return c


def _km_blocks(k, vals=None, rng=None):
    """k diagonal blocks of 2 columns x 4 rows: e0, e1, e0 + e1, e0 - e1 (or those supports with values drawn from vals)"""
    rows = []
    for b in range(k):
        rows += [{2 * b: 1}, {2 * b + 1: 1}, {2 * b: 1, 2 * b + 1: 1}, {2 * b: 1, 2 * b + 1: -1}]
    if vals:
        rows = [{j: _pick(rng, vals) for j in r} for r in rows]
    return rows


def kmethod_cases():
    """About 50 matrices at the limits of plo_kernel_search (128 rows, 64 columns, 64 dependent rows, rank 64, rows of 64
    entries, empty rows, eight moduli, 4 / 2 / 1 waves per workgroup) and seven it refuses.  Every case is scored as the
    (seed0, n) runs of SEED_RUNS with per_block = 1: plo_kernel_search takes a seed range only."""
    rng = random.Random(0x4B3E7)
    out = []
    # (a) the size limits on block-diagonal matrices: 4x2, 64x32, 68x34, 128x64 (rank 64 and 64 dependent rows), one row less,
    # and 64x32 with other values than +-1 (ProgramGen with one row per lane)
    for k in (1, 16, 17, 32):
        c = _km_case(out, "%dx%d" % (4 * k, 2 * k), "a", 2 * k, _km_blocks(k))
        assert (c.rank, c.m - c.rank) == (2 * k, 2 * k)
    c = _km_case(out, "127x64", "a", 64, _km_blocks(32)[:-1])
    assert (c.rank, c.m - c.rank) == (64, 63)
    c = _km_case(out, "64x32_vals", "a", 32, _km_blocks(16, [1, -1, 2, 3], rng))
    assert not c.unit and c.rank == 32
    # (b) few columns, many dependent rows
    c = _km_case(out, "65x1", "b", 1, [{0: _pick(rng, [1, -1])} for _ in range(65)])
    assert c.m - c.rank == 64
    c = _km_case(out, "66x2", "b", 2, [{0: 1}, {1: 1}] + [{0: 1, 1: _pick(rng, [1, -1])} for _ in range(64)])
    assert c.m - c.rank == 64
    vecs = [t for t in ((a, b, cc, d) for a in (0, 1, -1) for b in (0, 1, -1) for cc in (0, 1, -1) for d in (0, 1, -1)) if any(t)]
    c = _km_case(out, "68x4", "b", 4, [{j: v for j, v in enumerate(t) if v} for t in _sample(rng, vecs, 68)])
    assert (c.rank, c.m - c.rank) == (4, 64)
    c = _km_case(out, "40x3_rank1", "b", 3, [{0: k, 1: -k, 2: 2 * k} for k in (1 + rng.randrange(5) for _ in range(40))])
    assert c.rank == 1 and not c.unit
    # (c) long rows, and rows of Dep of every group width: the identity of size R and one row of R entries (its combination
    # has R entries and the rank is R: Dep's lpr_log2 = ceil(log2 R) goes from 2 to 6); R = 64 is a row of 64 entries
    for R in KM_R:
        eye = [{j: 1} for j in range(R)]
        _km_case(out, "R%d_ones" % R, "c", R, eye + [{j: 1 for j in range(R)}])
        if R + 1 <= 64:
            _km_case(out, "R%d_1toR" % R, "c", R, eye + [{j: j + 1 for j in range(R)}])
    c = _km_case(out, "64x16_dense", "c", 16, [{j: 1} for j in range(16)] + [{j: _pick(rng, [1, -1, 2]) for j in range(16)} for _ in range(48)])
    assert (c.m, c.rank) == (64, 16)
    # (d) degenerate rows and columns
    while True:
        rows = _rows(rng, 8, [2 + rng.randrange(2) for _ in range(12)], [1, -1, 2])
        if rank_mod(rows, KM_PRIME) == 8:
            break
    _km_case(out, "15x8_3empty", "d", 8, rows + [{}, {}, {}])
    _km_case(out, "3x2_empty", "d", 2, [{0: 1}, {1: 1}, {}])       # its only dependent row has an empty combination
    basis = [{0: 1, 1: -1}, {1: 1, 2: 1}, {2: -1, 3: 1}, {0: 1, 3: 1}]
    _km_case(out, "dup_unit", "d", 4, basis + [dict(basis[0]), dict(basis[2]), {j: -v for j, v in basis[1].items()}, dict(basis[0])])
    _km_case(out, "dup_twice", "d", 4, basis + [dict(basis[1]), {j: 2 * v for j, v in basis[2].items()}, {j: -2 * v for j, v in basis[0].items()}])
    while True:
        rows = [{2 * j: v for j, v in r.items()} for r in _rows(rng, 8, [2 + rng.randrange(2) for _ in range(12)], [1, -1, 2])]
        if rank_mod(rows, KM_PRIME) == 8:
            break
    _km_case(out, "12x16_even", "d", 16, rows)
    c = _km_case(out, "64x64_col63", "d", 64, _rows(rng, 64, [3] * 64, [1, -1, 2, 3], pool=list(range(63))), p=2147483629)
    assert c.rank < 64 and not c.unit
    # (e) moduli: both branches of kmul, p - 2 of every bit length in kinv, Barrett at 31 bits, on one 30x12 pattern
    pattern = _rows(rng, 12, [3] * 30, [1, -1, 2, 3, 6])
    for p in KM_MODULI:
        _km_case(out, "mod%d" % p, "e", 12, [{j: (v if v % p else 1) for j, v in r.items()} for r in pattern], p=p)
    # (f) the LDS choices: 112x56 block diagonal (the elimination arrays of 112 x 114 words and the combinations put a wave's
    # state between a third and a half of the LDS: two waves per workgroup); 4x2 has four, 128x64 one
    c = _km_case(out, "112x56", "f", 56, _km_blocks(28))
    assert (c.rank, c.m - c.rank) == (56, 56)
    # refusals, with the code include/plinopt_hip.h documents
    U = "PLO_E_UNSUPPORTED"
    _km_case(out, "67x2_65dep", "refuse", 2, [{0: 1}, {1: 1}] + [{0: 1, 1: _pick(rng, [1, -1])} for _ in range(65)], refusal=U)
    for s in range(1000):                                         # two +-1 entries per row: the seed that leaves rank 62, i.e. 66 dependent rows
        r2 = random.Random(0x4B3E7000 + s)
        rows = _rows(r2, 64, [2] * 128, [1, -1])
        if rank_mod(rows, KM_PRIME) == 62:
            break
    assert rank_mod(rows, KM_PRIME) == 62
    _km_case(out, "128x64_rank62", "refuse", 64, rows, refusal=U)
    _km_case(out, "129x2", "refuse", 2, [{0: 1}, {1: 1}] + [{0: 1, 1: _pick(rng, [1, -1])} for _ in range(127)], refusal=U)
    _km_case(out, "3x65", "refuse", 65, [{0: 1}, {64: 1}, {0: 1, 64: 1}], refusal=U)
    _km_case(out, "4x7_fullrank", "refuse", 7, [{0: 1, 4: 1}, {1: 1, 5: -1}, {2: 1, 6: 1}, {3: 1, 0: -1}], refusal=U)
    _km_case(out, "3x2_allempty", "refuse", 2, [{}, {}, {}], refusal=U)
    _km_case(out, "65x3_a2", "refuse", 3, [{0: 1}, {1: 1}, {2: 1}, {0: 1, 1: 2}] + _rows(rng, 3, [2] * 61, [1, -1]), refusal="PLO_E_CAPACITY")
    return out


# ---------------------------------------------------------------------------------------------------- trilinear
TRIL_RATS = [F(1), F(-1), F(1, 2), F(-2), F(3), F(-2, 3), F(1000003, 7)]
TRIL_VARIANTS = [("unit", UNIT, False), ("rat", TRIL_RATS, False), ("unit_e", UNIT, True), ("rat_e", TRIL_RATS, True)]
TRIL_SEEDS3 = [BASE_SEED, 0, (1 << 64) - 2]                      # the two programs near the 160 KiB of LDS
TRIL_TIE_N = 1000


def tril_layout(m, nnz, expanded):
    """(cap, lds_per_wave, waves per workgroup, LDS bytes of a workgroup) as plo_tril_plan_create_q sizes them; nnz of A, B, T"""
    cap = max(2 * z + 3 * m for z in nnz)
    if expanded:
        cap = max(cap, 4 * nnz[2] + 6 * m)
    cap = _ru(cap + 2, 64)
    per_wave = _ru(8 * cap + 2 * ((m + 1) & ~1) + m, 16) + 16 * ((cap + 63) // 64)
    waves = 4 if 4 * per_wave <= WG_LDS else 1
    return cap, per_wave, waves, waves * per_wave


def tril_refusal(m, mats, expanded):
    """None when the device takes the triple, else the name of the header's code (include/plinopt_hip.h, plo_tril_*), in the
    order plo_tril_plan_create_q checks; mats: three (n, entries)"""
    if m > 16382:
        return "PLO_E_CAPACITY"
    for w, (n, ent) in enumerate(mats):
        assert 0 < n <= 16382
        if len(ent) > 65535:
            return "PLO_E_CAPACITY"
        lens = [0] * m
        for (i, _), v in sorted(ent.items()):
            lens[i] += 1
        for i in range(m):
            if lens[i] == 0 or lens[i] > 64:
                return "PLO_E_UNSUPPORTED"
            if any(v.numerator % LIN_PRIME == 0 or v.denominator % LIN_PRIME == 0 for (r, _), v in ent.items() if r == i):
                return "PLO_E_UNSUPPORTED"
        if expanded and w == 2 and n >= 16382:
            return "PLO_E_CAPACITY"
    if tril_layout(m, [len(e) for _, e in mats], expanded)[3] > LDS_MAX:
        return "PLO_E_CAPACITY"
    return None


def tril_text(c):
    return "expanded %d\n" % c.expanded + "".join(sms_text(c.m, n, e) for n, e in c.mats)


def tril_quick(cap, unit):
    """The cases whose goldens tests/test_synth_golden.py recomputes, by a fixed rule on the program's capacity (the
    oracle's time follows the length of the longest of the three programs; rationals cost about twice as much)"""
    return cap * (1 if unit else 2) <= 6000


def _tril_case(out, name, family, m, mats, expanded, refusal=None, quick=None, seeds=None):
    """mats: three (n, rows) for A, B and T (the transposed product matrix), rows as {column: value}"""
    assert len(mats) == 3 and all(len(rows) == m and all(0 <= j < n for r in rows for j in r) for n, rows in mats), name
    ents = [(n, {(i, j): F(v) for i, r in enumerate(rows) for j, v in r.items()}) for n, rows in mats]
    got = tril_refusal(m, ents, expanded)
    assert got == refusal, (name, got)
    by_list = len(out) % 2 == 0 or seeds is not None
    unit = all(v in (1, -1) for _, e in ents for v in e.values())
    cap, per_wave, waves, lds = tril_layout(m, [len(e) for _, e in ents], expanded)
    c = SimpleNamespace(name="tril_%s_%s" % (family, name), family=family, m=m, mats=ents, expanded=bool(expanded), refusal=refusal,
                        mode="list" if by_list else "runs", seeds=list(seeds or (SEEDS_LIST if by_list else SEEDS_RUNS)), unit=unit,
                        cap=cap, lds_per_wave=per_wave, waves=waves, lds=lds, quick=(tril_quick(cap, unit) if quick is None else quick) and not refusal)
    c.sha256 = _sha(tril_text(c))
    assert c.name not in [x.name for x in out], c.name
    out.append(c)
    return c


def tril_args(c):
    """the three (n, rowptr, col, num, den) of plinopt_amd.TrilPlan"""
    return [qcsr(c.m, n, e)[1:] for n, e in c.mats]


def _spread(m, total):
    """row lengths that sum to total, as even as possible"""
    return [total // m + (1 if i < total % m else 0) for i in range(m)]


def tril_cases():
    """About 80 triples (A, B, T) at the edges of tril_kernel, t_linear with permutation and signs, t_double and
    t_pushvariables_ref, and six the device refuses.  Every row is non-empty."""
    rng = random.Random(0x7A11)
    out = []
    short = lambda m, n, vals: _rows(rng, n, [1 + rng.randrange(min(3, n)) for _ in range(m)], vals)  # noqa: E731
    # (a) row-count edges with 3..9 variables per matrix, the three counts different
    for m in (1, 2, 63, 64, 65, 129):
        for fl, vals, ex in TRIL_VARIANTS:
            ns = _sample(rng, range(3, 10), 3)
            _tril_case(out, "m%d_%s" % (m, fl), "a", m, [(n, short(m, n, vals)) for n in ns], ex)
    # (b) row lengths: a row of 64 entries in A only, in B only, in T only and in all three (20 rows, 64 variables), every row
    # of length 1, and a single row of 64 entries under -e
    for where in ("A", "B", "T", "ABT"):
        for fl, vals, ex in TRIL_VARIANTS:
            mats = []
            for x in "ABT":
                lens = [1 + rng.randrange(4) for _ in range(20)]
                if x in where:
                    lens[rng.randrange(20)] = 64
                mats.append((64, _rows(rng, 64, lens, vals)))
            _tril_case(out, "row64_%s_%s" % (where, fl), "b", 20, mats, ex)
    for fl, vals, ex in TRIL_VARIANTS:
        _tril_case(out, "len1_%s" % fl, "b", 12, [(n, _rows(rng, n, [1] * 12, vals)) for n in (5, 7, 4)], ex)
    for fl, vals, ex in TRIL_VARIANTS[2:]:
        _tril_case(out, "m1_T64_%s" % fl, "b", 1, [(3, _rows(rng, 3, [2], vals)), (4, _rows(rng, 4, [3], vals)), (64, _rows(rng, 64, [64], vals))], ex)
    # (c) the row forms of t_double (expanded only): the row's first column i with column i + 1 present and absent, pivot +-1,
    # 3 and 1/2, the first entry in the last column, single-entry rows of each kind
    for fl, vals, piv in (("unit_e", UNIT, [F(1), F(-1), F(-1), F(1)]), ("rat_e", TRIL_RATS, [F(1), F(-1), F(3), F(1, 2)])):
        v = lambda: _pick(rng, vals)  # noqa: E731
        T = []
        for a in piv:
            T += [{2: a, 3: v(), 5: v()}, {1: a, 4: v(), 6: v()}, {5: a, 6: v()}, {0: a, 7: v()}, {7: a}, {3: a}, {6: a, 7: v()}]
        m = len(T)
        _tril_case(out, "forms_%s" % fl, "c", m, [(5, short(m, 5, vals)), (6, short(m, 6, vals)), (8, T)], True)
    # (d) variable indices: the 14-bit src/des fields of the rational atom next to the "none" code 0x3FFF
    for fl, vals, ex in TRIL_VARIANTS:
        mats = []
        for n in (16382, 16382, 16381 if ex else 16382):
            pool = [0, 1, n // 2, n - 3, n - 2, n - 1]
            rows = [{0: vals[0], n - 1: vals[1], n - 2: vals[0]}, {n - 1: vals[1], 1: vals[0], 0: vals[1]}] + _rows(rng, n, [3] * 10, vals, pool)
            mats.append((n, rows))
        _tril_case(out, "n16382_%s" % fl, "d", 12, mats, ex)
    # (e) LDS: four waves of a workgroup just under and just over 64 KiB (the switch to one wave per workgroup), 300x64 and
    # 200x64, and two programs near the 160 KiB of a CU
    for fl, vals, ex in TRIL_VARIANTS:
        for side, tot in (("under", 320 if ex else 800), ("over", 336 if ex else 832)):
            lens = {"A": _spread(100, 300), "B": _spread(100, 300), "T": _spread(100, 300)}
            lens["T" if ex else "A"] = _spread(100, tot)
            c = _tril_case(out, "%s64k_%s" % (side, fl), "e", 100, [(40, _rows(rng, 40, lens[x], vals)) for x in "ABT"], ex)
            assert c.waves == (4 if side == "under" else 1) and abs(4 * c.lds_per_wave - WG_LDS) < 1200, (c.name, c.lds_per_wave)
    c = _tril_case(out, "300x64_unit", "e", 300, [(64, _rows(rng, 64, [1 + rng.randrange(4) for _ in range(300)], UNIT)) for _ in range(3)], False)
    assert c.waves == 1
    c = _tril_case(out, "200x64_rat_e", "e", 200, [(64, _rows(rng, 64, [1 + rng.randrange(4) for _ in range(200)], TRIL_RATS)) for _ in range(3)], True)
    assert c.waves == 1
    c = _tril_case(out, "1200x200_unit", "e", 1200, [(200, _rows(rng, 200, [5] * 1200, UNIT)) for _ in range(3)], False, quick=False, seeds=TRIL_SEEDS3)
    assert c.waves == 1 and 128 * 1024 < c.lds <= LDS_MAX
    c = _tril_case(out, "600x200_rat_e", "e", 600, [(200, _rows(rng, 200, [5] * 600, TRIL_RATS)) for _ in range(3)], True, quick=False, seeds=TRIL_SEEDS3)
    assert c.waves == 1 and 127 * 1024 < c.lds <= LDS_MAX
    assert all(c.waves == 4 for c in out if c.family in "abcd")
    # refusals
    ok = lambda m, n: _rows(rng, n, [2] * m, UNIT)  # noqa: E731
    U, C = "PLO_E_UNSUPPORTED", "PLO_E_CAPACITY"
    _tril_case(out, "empty_row", "refuse", 4, [(5, ok(4, 5)), (5, _rows(rng, 5, [2, 0, 1, 2], UNIT)), (5, ok(4, 5))], False, refusal=U)
    _tril_case(out, "row65", "refuse", 3, [(70, ok(3, 70)), (70, ok(3, 70)), (70, _rows(rng, 70, [2, 65, 3], UNIT))], False, refusal=U)
    _tril_case(out, "T16382_e", "refuse", 3, [(5, ok(3, 5)), (5, ok(3, 5)), (16382, [{0: 1, 16381: -1}, {1: 1}, {16380: 1, 16381: 1}])], True, refusal=C)
    _tril_case(out, "num_prime", "refuse", 3, [(5, [{0: 1, 1: F(LIN_PRIME, 3)}, {2: 1}, {3: -1}]), (5, ok(3, 5)), (5, ok(3, 5))], False, refusal=U)
    _tril_case(out, "den_prime", "refuse", 3, [(5, ok(3, 5)), (5, ok(3, 5)), (5, [{0: 1}, {2: F(2, LIN_PRIME)}, {3: -1}])], True, refusal=U)
    _tril_case(out, "m16383", "refuse", 16383, [(5, _rows(rng, 5, [1] * 16383, UNIT)) for _ in range(3)], False, refusal=C)
    return out


def tril_tie_cases():
    """two tiny triples whose candidates tie all the time: the argmin under (ADD, SCA, seed, variant)"""
    rng = random.Random(0x71E7)
    out = []
    _tril_case(out, "2x2_unit", "tie", 2, [(2, _rows(rng, 2, [2, 1], UNIT)), (2, _rows(rng, 2, [1, 2], UNIT)), (2, _rows(rng, 2, [2, 2], UNIT))], False)
    _tril_case(out, "3x3_rat_e", "tie", 3, [(3, _rows(rng, 3, [2, 1, 2], TRIL_RATS)), (2, _rows(rng, 2, [1, 2, 1], TRIL_RATS)), (3, _rows(rng, 3, [2, 2, 1], TRIL_RATS))], True)
    return out


# ======================================================================================================================
# Edge-shape cases for the chained-candidate kernels (plo_cse_wave.hip cse_chain_kernel through plo_cse_chain_*, and
# cse_chain_batch_kernel through plo_cse_chain_batch): two matrices per candidate, one random stream.  No golden file: the
# oracle (oracle/plo_oracle.c plo_oracle_chain) scores them in milliseconds, tests/test_chain_cases_host.py holds the family
# to what it is meant to distinguish and tests/test_gpu_chain_synth.py the kernels to the oracle.
#
# wave_plan() restates the admission rules and the LDS layout of build_plan / layout_wave_image (plo_capi.hip), so that
# every case is checked HERE to be taken or refused as it says, and to have the layout property it is there for.
# ======================================================================================================================
CHAIN_PRIME = 131071
CHAIN_MODULI = [3, 7, 101, 2147483629, 2147483647]
CHAIN_RUN = (0, 8)                                               # scored as one (seed0, n) run ...
CHAIN_SEEDS = [2 ** 40, 2 ** 63, 2 ** 64 - 1, 5, 5]              # ... and as one explicit list: above 2^32, and one seed twice


def wave_plan(m, n, rows, p, cap_scale=2, tight=False):
    """The name of the header's code when build_plan refuses the matrix for the LDS-resident wave kernel, else its plan: mw,
    unit, NC, distinct initial triples, cap, and tmpl_bytes / region_bytes / rs_bytes of layout_wave_image.  tight: the
    table of the PLO_WAVE_CAP_TIGHT knob."""
    rows = [{j: v % p for j, v in r.items() if v % p} for r in rows]
    nnz, maxlen = sum(len(r) for r in rows), max([len(r) for r in rows] + [0])
    unit = all(v in (1 % p, p - 1) for r in rows for v in r.values())
    if maxlen > 64 or m == 0 or m > 31 * 64:
        return "PLO_E_CAPACITY"
    mw = (m + 63) // 64
    if not unit and mw > 1:
        return "PLO_E_CAPACITY"
    naive = sum(max(len(r) - 1, 0) for r in rows)
    NC = n + naive // 2 + 2
    if NC >= 0xFFFF or 2 * _clog2(NC) + _clog2(p) > 51 or 2 * nnz >= 65535:
        return "PLO_E_CAPACITY"
    triples = {}
    for r in rows:
        e = sorted(r.items())
        for x in range(len(e)):
            for y in range(x + 1, len(e)):
                k = (e[x][0], e[y][0], e[y][1] * pow(e[x][1], -1, p) % p)
                triples[k] = triples.get(k, 0) + 1
    cap = 64
    if tight:
        while cap < len(triples) + 1:
            cap *= 2
        cap *= cap_scale // 2
    else:
        while cap < 2 * len(triples) * 3 // 4 + 16:
            cap *= 2
        cap *= cap_scale // 2                                    # every repeat has twice the slots
    if cap > 65536:
        return "PLO_E_CAPACITY"
    multcap = 0 if unit else naive // 2 + 8
    off = _ru(cap * 8 + nnz * (6 if unit else 10) + m * 2, 8)
    tmpl = off + n * 2 * mw * 8
    off += NC * 2 * mw * 8 + (2 * mw + 1) * 8 + cap * 2
    region = _ru(_ru(off, 8) + multcap * 8, 16)
    rs = _ru((m + 1) * 2, 16)
    if rs + region > LDS_MAX:
        return "PLO_E_CAPACITY"
    return SimpleNamespace(mw=mw, unit=unit, NC=NC, distinct=len(triples), maxfreq=max(list(triples.values()) + [0]), cap=cap,
                           tmpl_bytes=tmpl, region_bytes=region, rs_bytes=rs)


def pick_waves(lds, limit=LDS_MAX):
    """(waves per workgroup, LDS bytes) as pick_waves(most_per_cu = true) of plo_capi.hip chooses among 4, 2 and 1"""
    W = best = got = 0
    for w in (4, 2, 1):
        if lds(w) > limit:
            continue
        waves = min(32, limit // lds(w) * w)
        if W and waves <= best:
            continue
        W, best, got = w, waves, lds(w)
    return W, got


def chain_layout(A, B):
    """(waves per workgroup, LDS bytes) of chain_config for two admitted plans"""
    return pick_waves(lambda w: A.rs_bytes + B.rs_bytes + w * max(A.region_bytes, B.region_bytes))


def _chain_case(out, name, family, A, B, p=CHAIN_PRIME, refusal=None, run=CHAIN_RUN, seeds=CHAIN_SEEDS):
    """A, B: (columns, rows) with rows as {column: signed value}; the case holds the residues"""
    mats, plans = [], []
    for n, rows in (A, B):
        assert all(0 <= j < n and v % p for r in rows for j, v in r.items()), name
        rows = [{j: v % p for j, v in r.items()} for r in rows]
        assert sum(len(r) for r in rows) <= 1100 or family == "onewave" or refusal, name        # (the oracle's time; it never sees a refused pair)
        mats.append(SimpleNamespace(m=len(rows), n=n, rows=rows, csr=(len(rows), n) + to_csr(rows, p)))
        plans.append(wave_plan(len(rows), n, rows, p))
    got = next((x for x in plans if isinstance(x, str)), None)
    if got is None and chain_layout(*plans)[0] == 0:
        got = "PLO_E_CAPACITY"
    assert got == refusal, (name, got)
    c = SimpleNamespace(name="chain_%s_%s" % (family, name), family=family, A=mats[0], B=mats[1], p=p, refusal=refusal, run=run, seeds=list(seeds),
                        plans=plans, silent_first=not refusal and plans[0].maxfreq <= 1, relaunch=False,
                        waves=None if refusal else chain_layout(*plans)[0], lds=None if refusal else chain_layout(*plans)[1])
    assert c.name not in [x.name for x in out], c.name
    out.append(c)
    return c


def _dense(rng, m, n, vals, density=1.0):
    return n, [{j: _pick(rng, vals) for j in range(n) if density >= 1.0 or rng.random() < density} for _ in range(m)]


CHAIN_ORDER_A = (6, [{0: 1, 1: -1, 2: 1, 3: 1, 4: -1, 5: 1}, {0: 1, 1: 1, 2: -1, 3: 1, 4: 1, 5: -1}, {0: -1, 1: 1, 2: 1, 3: -1, 4: 1, 5: 1},
                     {0: 1, 1: 1, 2: 1, 3: 1, 4: 1, 5: 1}, {0: 1, 1: -1, 2: -1, 3: 1, 4: -1, 5: -1}, {0: -1, 1: -1, 2: 1, 3: 1, 4: 1, 5: -1},
                     {0: 1, 1: 1, 2: -1, 3: -1, 4: 1, 5: 1}, {0: -1, 1: 1, 2: -1, 3: 1, 4: -1, 5: 1}])


def chain_cases():
    """About 50 pairs of matrices at the edges of cse_chain_kernel and cse_chain_batch_kernel: what the second run_candidate
    finds in the LDS region the first one left, the four unit/general dispatches, first matrices that draw nothing from the
    random stream, more than 64 rows, rows of 64 entries, moduli from 3 to 2^31 - 1, one wave per workgroup, and four pairs
    the chain refuses.  The table of the 150 x 6 matrix (30 initial triples, 64 slots) fills up under the usual sizing: its two
    pairs take the table-full relaunch without any knob (c.relaunch)."""
    rng = random.Random(0xC4A15)
    out = []
    GEN = [1, -1, 2, 3]
    tiny = (3, [{0: 1, 1: 2, 2: 1}, {0: 1, 1: 2}, {1: -1, 2: 3}])
    # order: the same two matrices both ways round; every tie of the first moves the stream the second sees
    gen7x5 = _dense(rng, 7, 5, GEN)
    gen9x6 = _dense(rng, 9, 6, [1, -1, 2, -2, 3], 0.8)
    gen8x7 = _dense(rng, 8, 7, GEN, 0.8)
    for name, A, B in (("u8x6_g7x5", CHAIN_ORDER_A, gen7x5), ("g9x6_g8x7", gen9x6, gen8x7)):
        _chain_case(out, name, "order", A, B)
        _chain_case(out, name + "_rev", "order", B, A)
    # dispatch: P.unit is read per matrix at run time, all four combinations at 6 and at 12 rows
    for m in (6, 12):
        for fa, va in (("unit", [1, -1]), ("gen", GEN)):
            for fb, vb in (("unit", [1, -1]), ("gen", GEN)):
                c = _chain_case(out, "%s_%s_%d" % (fa, fb, m), "dispatch", _dense(rng, m, 5 + m // 6, va, 0.85), _dense(rng, m - 1, 4 + m // 6, vb, 0.85))
                assert [x.unit for x in c.plans] == [fa == "unit", fb == "unit"]
    # silent first: matrices that draw nothing from the stream (no pair at all, or no pair of frequency 2), and the -K host
    # decomposition's emptied rows (which does draw), each before and after a matrix that draws
    draws = _dense(rng, 8, 6, GEN)
    freq1 = (5, [{0: 1, 1: 2, 2: 3}, {0: 1, 1: 5, 3: 7}, {1: 1, 2: 11, 4: 13}, {0: 2, 3: 17, 4: 19}, {2: 1, 3: 23}])
    holes = _dense(rng, 11, 6, GEN)
    for i in (0, 4, 5, 10):
        holes[1][i] = {}
    for name, S, silent in (("empty3x2", (2, [{}, {}, {}]), True), ("1x1", (1, [{0: 2}]), True), ("freq1", freq1, True), ("emptied_rows", holes, False)):
        c = _chain_case(out, name + "_first", "silent", S, draws)
        assert c.silent_first == silent and c.plans[1].maxfreq > 1
        c = _chain_case(out, name + "_second", "silent", draws, S)
        assert not c.silent_first
    # region dominance: the region is max(region_bytes), and only tmpl_bytes of the second image are rewritten
    big = _dense(rng, 40, 32, [1, -1, 2], 0.8)
    c = _chain_case(out, "big_tiny", "region", big, tiny)
    assert c.plans[0].region_bytes > 8 * c.plans[1].region_bytes
    _chain_case(out, "tiny_big", "region", tiny, big)
    pool = [0, 1, 2, 650, 651, 1297, 1298, 1299]
    wide = (1300, [{j: _pick(rng, [1, -1]) for j in _sample(rng, pool, 3)} for _ in range(16)])              # 1300 columns, 128 slots
    deep = _dense(rng, 30, 8, list(range(2, 40)))                                                            # 8 columns, some 800 triples
    for name, A, B in (("wide_deep", wide, deep), ("deep_wide", deep, wide)):
        c = _chain_case(out, name, "region", A, B)
        w, d = c.plans if A is wide else c.plans[::-1]
        assert w.tmpl_bytes > d.tmpl_bytes and w.region_bytes < d.region_bytes and w.cap < d.cap
    # mw > 1 (more than 64 rows, +-1 only) next to a general matrix, and mw 2 next to mw 3
    gen20 = _dense(rng, 20, 6, GEN, 0.7)
    for m, n in ((65, 3), (150, 6)):
        U = _dense(rng, m, n, [1, -1], 0.9)
        c = _chain_case(out, "%dx%d_gen" % (m, n), "mw", U, gen20)
        assert [x.mw for x in c.plans] == [(m + 63) // 64, 1]
        c.relaunch = m == 150
        _chain_case(out, "gen_%dx%d" % (m, n), "mw", gen20, U).relaunch = m == 150
    c = _chain_case(out, "128x4_129x4", "mw", _dense(rng, 128, 4, [1, -1], 0.9), _dense(rng, 129, 4, [1, -1], 0.9))
    assert [x.mw for x in c.plans] == [2, 3]
    # row length: rows of 64 entries (lpr_log2 = 6: one row per wave trip)
    u2x64, u6x64 = _dense(rng, 2, 64, [1, -1]), _dense(rng, 6, 64, [1, -1])
    _chain_case(out, "2x64_gen", "rowlen", u2x64, gen20)
    _chain_case(out, "6x64_2x64", "rowlen", u6x64, u2x64)
    _chain_case(out, "gen_6x64", "rowlen", gen20, u6x64)
    g3x64 = _dense(rng, 3, 64, [1, -1, 2, 3, 4])
    for p in (3, 7):
        fix = (64, [{j: (v if v % p else 1) for j, v in r.items()} for r in g3x64[1]])
        c = _chain_case(out, "3x64_mod%d" % p, "rowlen", fix, (6, [{j: (v if v % p else 1) for j, v in r.items()} for r in gen20[1]]), p=p)
        assert c.plans[0].unit == (p == 3)                       # at p = 3 every residue is +-1
    _chain_case(out, "gen2x64_tiny", "rowlen", (64, g3x64[1][:2]), tiny)     # (three such rows at this modulus: 6048 triples, past the LDS)
    # moduli: rb and the key layout of both plans, one unit/general pair both ways round
    mu, mg = _dense(rng, 10, 7, [1, -1], 0.8), _dense(rng, 9, 6, [1, -1, 2, 3, 5, 6], 0.8)
    for p in CHAIN_MODULI:
        g = (mg[0], [{j: (v if v % p else 1) for j, v in r.items()} for r in mg[1]])
        _chain_case(out, "unit_gen_mod%d" % p, "moduli", mu, g, p=p)
        _chain_case(out, "gen_unit_mod%d" % p, "moduli", g, mu, p=p)
    # one wave per workgroup: the largest dense +-1 square that runs with one wave, 60 x 60 (3540 triples, 8192 slots, 130 KB of the
    # 160 KiB).  The live triples of such a matrix grow to 2.2 times the initial ones: 64 x 64 and 62 x 62 fill the 8192 slots, which
    # cannot be doubled inside the LDS, 61 x 61 comes within 2 % of them, 52 x 52 and smaller have 4096 slots and two waves.  The
    # oracle takes most of a second per seed: three seeds, the list repeats them
    c = _chain_case(out, "60x60_tiny", "onewave", _dense(rng, 60, 60, [1, -1]), tiny, run=(0, 3), seeds=[2, 0, 2])
    assert c.waves == 1 and c.plans[0].cap == 8192 and 128 * 1024 < c.lds <= LDS_MAX
    assert all(c.waves == 4 for c in out if c.family in ("order", "dispatch", "silent", "moduli"))
    # refusals: plans of the HBM family (a +-1 matrix of 1984 rows whose masks alone pass 160 KiB; more than 64 rows with another
    # coefficient than +-1), as first and as second matrix
    C = "PLO_E_CAPACITY"
    u1984 = _dense(rng, 1984, 2, [1, -1])
    g65 = (2, [{0: 1, 1: 2}] + [{0: _pick(rng, [1, -1]), 1: _pick(rng, [1, -1])} for _ in range(64)])
    assert wave_plan(1984, 2, u1984[1], CHAIN_PRIME) == C and wave_plan(65, 2, g65[1], CHAIN_PRIME) == C
    _chain_case(out, "1984x2_first", "refuse", u1984, tiny, refusal=C)
    _chain_case(out, "1984x2_second", "refuse", tiny, u1984, refusal=C)
    _chain_case(out, "gen65x2_first", "refuse", g65, tiny, refusal=C)
    _chain_case(out, "gen65x2_second", "refuse", tiny, g65, refusal=C)
    return out


# ======================================================================================================================
# Edge-shape cases for the one-wave CSE kernel itself (plo_cse_wave.hip run_candidate / program_gen_general through CSEPlan:
# cost_many, search, the -E walk and the plan's own table-full relaunch).  No golden costs: the oracle (oracle/plo_oracle.c)
# scores every case in milliseconds, tests/test_cse_cases_host.py holds each case to the property it was built for and
# tests/test_gpu_cse_edges.py the kernel to the oracle; tests/golden/cse_cases.json pins names, shapes and matrices.
#
# Every case states the branch boundary it sits on and asserts it here, from the matrix alone: the number of triples of
# maximal frequency (the tie pick's three paths: 1, <= 64, > 64), the rows that hold both columns of the first step against
# G = 64 >> lpr_log2 (one trip or the two sweeps), the (column, |v|) keys of ProgramGen against the slots of the pair table
# they share, the mask words, the row-length class, the key width.  Where a property needed a search over generator seeds
# (22 x 40 matrices of maximal frequency 2 with 63..66 tied triples are some 0.01 % of the seeds) the seed found is the
# constant below.
# ======================================================================================================================
CSE_PRIME = CHAIN_PRIME
CSE_MODULI = [3, 5, 7, 65521, 65537, 2147483629, 2147483647]
CSE_RUN, CSE_TIE_RUN = (0, 8), (0, 16)                           # the (seed0, n) run: 16 seeds where the costs must vary
CSE_SEEDS = [2 ** 64 - 1, 2 ** 63, 2 ** 40 + 7, 5, 5]            # the explicit list: the ends, above 2^40, one seed twice
CSE_ENUM = 64                                                    # schedule indices walked from 0 and from CSE_ENUM_FAR
CSE_ENUM_FAR = 10 ** 12 + 12345
CSE_GEN = [1, -1, 2, 3]
CSE_TIE_SEED = 0xC5E0000                                         # 22 x 40, seven +-1 per row: offset -> tied triples (frequency 2)
CSE_TIE_UNIT = {63: 1510, 64: 60977, 65: 5083, 66: 42557}
CSE_TIE_BLOCKS = {128: (3821, 58750), 129: (10684, 58750)}       # two such blocks on the diagonal: 60 + 68 and 61 + 68
CSE_TIE_GEN_SEED, CSE_TIE_GEN = 0xC5E6000, {63: 1, 64: 2, 65: 1, 66: 3}   # the general construction: the first draws whose costs take five values over 16 seeds
CSE_TIE_FEW = {1: 0xC5E1000 + 7919 * 12, 2: 0xC5E1000 + 7919 * 12 + 51}   # 12 x 40: one and two triples of frequency 3


def cse_triples(rows, p):
    """{(column a, column b, ratio): rows that hold it} of the initial pair table (listpairs), a < b"""
    t = {}
    for r in rows:
        e = sorted((j, v % p) for j, v in r.items() if v % p)
        for x in range(len(e)):
            for y in range(x + 1, len(e)):
                k = (e[x][0], e[y][0], e[y][1] * pow(e[x][1], -1, p) % p)
                t[k] = t.get(k, 0) + 1
    return t


def cse_top(rows, p):
    """(maximal frequency, the triples that have it in map order)"""
    t = cse_triples(rows, p)
    mf = max(list(t.values()) + [0])
    return mf, sorted(k for k, v in t.items() if v == mf)


def cse_group(maxlen):
    """(lpr_log2, G): lanes per row and rows per trip of the sweeps, as build_plan sets them from the longest row"""
    lpr = max(2, _clog2(max(maxlen, 1)))
    return lpr, 64 >> lpr


def cse_pgen_keys(rows, p):
    """the (column, |v|) keys that ProgramGen's pass A1 inserts into the pair table's slots when no CSE step ran before"""
    return {(j, min(v % p, p - v % p)) for r in rows for j, v in r.items() if v % p not in (0, 1, p - 1)}


def _cse_case(out, name, family, n, rows, p=CSE_PRIME, run=CSE_RUN, enum=0, refusal=None, **prop):
    """rows: one {column: signed value} per row; the case holds the residues.  prop: what the case was built for"""
    m = len(rows)
    assert all(0 <= j < n and v % p for r in rows for j, v in r.items()), name
    rows = [{j: v % p for j, v in r.items()} for r in rows]
    plan = wave_plan(m, n, rows, p)
    assert (plan if isinstance(plan, str) else None) == refusal, (name, plan)
    mf, top = cse_top(rows, p)
    maxlen = max(len(r) for r in rows)
    lpr, G = cse_group(maxlen)
    c = SimpleNamespace(name="cse_%s_%s" % (family, name), family=family, m=m, n=n, rows=rows, p=p, csr=(m, n) + to_csr(rows, p), plan=plan,
                        hbm=refusal is not None, run=run, seeds=[] if refusal else list(CSE_SEEDS), enum=enum, maxfreq=mf, T=len(top), top=top,
                        maxlen=maxlen, lpr_log2=lpr, G=G, keys=len(cse_pgen_keys(rows, p)), prop=prop, sha256=_sha(km_text(m, n, p, rows)))
    assert not (enum and refusal) and c.name not in [x.name for x in out], c.name
    out.append(c)
    return c


def _unit_rows(seed, m, n=40, k=7, shift=0):
    rng = random.Random(seed)
    return [{shift + j: _pick(rng, [1, -1]) for j in _sample(rng, range(n), k)} for _ in range(m)]


def _holders(rows, a, b):
    return [i for i, r in enumerate(rows) if a in r and b in r]


def _forced(c, share, ratio):
    """the first step is forced: (0, 1, ratio) is the only triple of frequency >= 2, and `share` rows hold it"""
    t = cse_triples(c.rows, c.p)
    assert c.top == [(0, 1, ratio % c.p)] and c.maxfreq == share and sorted(t.values())[-2] == 1, c.name


def _group_rows(rng, L, share, vals, ratio, other=None):
    """`share` rows of L entries with columns 0 and 1 at `ratio`, the other L - 2 entries of each row in columns of its own;
    other: the ratio of one more row that holds both columns, put in the middle of the rows"""
    rows, n = [], 2
    for i in range(share + (other is not None)):
        u = _pick(rng, vals)
        r = {0: u, 1: u * (other if other is not None and i == share // 2 else ratio)}
        for _ in range(L - 2):
            r[n] = _pick(rng, vals)
            n += 1
        rows.append(r)
    return n, rows


def _near_rows(rng, k, vals):
    """k rows of 64 entries over the same 64 columns that differ from the first in three entries each"""
    base = {j: _pick(rng, vals) for j in range(64)}
    rows = [dict(base)]
    for _ in range(k - 1):
        r = dict(base)
        for j in _sample(rng, range(64), 3):
            r[j] = -r[j]
        rows.append(r)
    return 64, rows


def _factor_rows():
    """two rows over 64 columns without one triple in common (the quotients r1[j] / r0[j] are pairwise distinct, so no CSE step
    runs), no (column, |v|) twice, every |v| of 2..9 several times in each row and under both signs: FactorOutRows at LPR = 64"""
    vals = [s * a for a in range(2, 10) for s in (1, -1)]
    every = [(x, y) for x in vals for y in vals if abs(x) != abs(y)]
    random.Random(0xFAC7).shuffle(every)
    pairs, seen = [], set()
    for x, y in every:
        if F(y, x) not in seen and len(pairs) < 64:
            seen.add(F(y, x))
            pairs.append((x, y))
    assert len(pairs) == 64
    rows = [{j: xy[0] for j, xy in enumerate(pairs)}, {j: xy[1] for j, xy in enumerate(pairs)}]
    for r in rows:
        for a in range(2, 10):
            assert sum(v == a for v in r.values()) >= 1 and sum(v == -a for v in r.values()) >= 1 and sum(abs(v) == a for v in r.values()) >= 3, (a, r)
    return 64, rows


def cse_cases():
    """89 matrices at the branch boundaries of run_candidate and program_gen_general, two of them sent to the HBM family."""
    rng = random.Random(0xC5E)
    out = []
    P = CSE_PRIME
    # ---- tie: the triples of maximal frequency at the start: 1, 2 (rank by readlane), 63, 64 (a full wave of ties), 65, 66, 128, 129
    # (bisection on the key, tie list in blocks of 64).  +-1: random rows; the costs vary with the seed.  -E on 63/64/65: the
    # maximal frequency is 2, so the children of the root are these same triples
    for T, s in sorted(CSE_TIE_FEW.items()):
        c = _cse_case(out, "unit_T%d" % T, "tie", 40, _unit_rows(s, 12), run=CSE_TIE_RUN)
        assert (c.T, c.maxfreq) == (T, 3), (c.name, c.T, c.maxfreq)
    for T, s in sorted(CSE_TIE_UNIT.items()):
        c = _cse_case(out, "unit_T%d" % T, "tie", 40, _unit_rows(CSE_TIE_SEED + s, 22), run=CSE_TIE_RUN, enum=CSE_ENUM if T <= 65 else 0)
        assert (c.T, c.maxfreq) == (T, 2), (c.name, c.T, c.maxfreq)
    for T, (s1, s2) in sorted(CSE_TIE_BLOCKS.items()):
        c = _cse_case(out, "unit_T%d" % T, "tie", 80, _unit_rows(CSE_TIE_SEED + s1, 22) + _unit_rows(CSE_TIE_SEED + s2, 22, shift=40), run=CSE_TIE_RUN)
        assert (c.T, c.maxfreq) == (T, 2), (c.name, c.T, c.maxfreq)
    # general: two identical rows of 11 entries (55 triples of frequency 2) and k - 55 identical pairs of two-entry rows in columns of their own
    for k, s in sorted(CSE_TIE_GEN.items()):
        r2 = random.Random(CSE_TIE_GEN_SEED + 100 * k + s)
        first = {j: _pick(r2, [2, 3, -2, 1]) for j in range(11)}
        rows, n = [dict(first), dict(first)], 11
        for _ in range(k - 55):
            r = {n: _pick(r2, [2, 3, -2, 1]), n + 1: _pick(r2, [2, 3, -2, 1])}
            rows += [dict(r), dict(r)]
            n += 2
        c = _cse_case(out, "gen_T%d" % k, "tie", n, rows, run=CSE_TIE_RUN, enum=CSE_ENUM if k <= 65 else 0)
        assert (c.T, c.maxfreq) == (k, 2) and not c.plan.unit, (c.name, c.T, c.maxfreq)
    # ---- group: the first step rewrites exactly G, and exactly G + 1, rows (G = 64 >> lpr_log2 rows per trip: at most G rows holding
    # both columns take the one-trip path, more the two sweeps).  The step is forced.  General: one more row holds both columns at
    # another ratio (in the mask, not rewritten), so G rows of the triple already take the sweeps; Gm1 is the one-trip path with such a row
    for L in (4, 8, 16, 32):
        lpr, G = cse_group(L)
        for share, tag in ((G, "G"), (G + 1, "G1")):
            n, rows = _group_rows(rng, L, share, [1, -1], 1)
            c = _cse_case(out, "L%d_unit_%s" % (L, tag), "group", n, rows, share=share, mask=share)
            _forced(c, share, 1)
            assert c.G == G and c.maxlen == L and len(_holders(c.rows, 0, 1)) == share and c.plan.unit
        for share, tag in ((G - 1, "Gm1"), (G, "G"), (G + 1, "G1")):
            if share < 2:
                continue
            n, rows = _group_rows(rng, L, share, [1, -1, 2, -2], 3, other=2)
            c = _cse_case(out, "L%d_gen_%s" % (L, tag), "group", n, rows, share=share, mask=share + 1)
            _forced(c, share, 3)
            assert c.G == G and c.maxlen == L and len(_holders(c.rows, 0, 1)) == share + 1 and not c.plan.unit
    # L = 64: G = 1, every step takes the sweeps, one row per trip.  (Rows of 64 entries in columns of their own do not fit the LDS.)
    for k in (2, 3):
        for fl, vals in (("unit", [1, -1]), ("gen", CSE_GEN)):
            c = _cse_case(out, "L64_%s_%drows" % (fl, k), "group", *_near_rows(rng, k, vals), share=k, mask=k)
            assert c.G == 1 and c.maxlen == 64 and c.maxfreq == k and c.plan.unit == (fl == "unit")
    # ---- rowlen: the lpr_log2 classes at their boundaries, and a row count that is no multiple of G: the last trip of the r0 += G
    # loops (ProgramGen) is partial.  A row of 65 entries goes to the HBM family
    for L, m in ((4, 19), (5, 11), (8, 11), (9, 7), (16, 7), (17, 5), (32, 5), (33, 3), (64, 3)):
        lpr, G = cse_group(L)
        lens = [max(2, L - i * L // m) for i in range(m)]
        for fl, vals in (("unit", [1, -1]), ("gen", CSE_GEN)):
            c = _cse_case(out, "L%d_%s" % (L, fl), "rowlen", L + 2, _rows(rng, L + 2, lens, vals))
            assert c.maxlen == L and (c.lpr_log2, c.G) == (lpr, G) and (G == 1 or m % G) and c.maxfreq >= 2 and c.plan.unit == (fl == "unit")
    assert sorted({c.lpr_log2 for c in out if c.family == "rowlen"}) == [2, 3, 4, 5, 6]
    c = _cse_case(out, "L65_unit", "rowlen", 70, _rows(rng, 70, [65, 3, 2], [1, -1]), refusal="PLO_E_CAPACITY")
    assert c.maxlen == 65
    # ---- mw: +-1 matrices of 63 .. 129 rows (one, two and three mask words), and one whose first step rewrites 40 rows: 34 in word 0
    # up to row 63 (more than G = 8 of them: several trips inside a word) and 6 in word 1 from row 64
    for m in (63, 64, 65, 128, 129):
        c = _cse_case(out, "%dx5" % m, "mw", *_dense(rng, m, 5, [1, -1], 0.8))
        assert c.plan.mw == (m + 63) // 64 and c.plan.unit
    rows = []
    for i in range(100):
        r = {j: _pick(rng, [1, -1]) for j in range(2, 7) if rng.random() < 0.6}
        if 30 <= i < 70:
            r[0] = r[1] = _pick(rng, [1, -1])
        rows.append(r)
    c = _cse_case(out, "straddle_100x7", "mw", 7, rows, share=40)
    held = _holders(c.rows, 0, 1)
    assert c.top == [(0, 1, 1)] and c.maxfreq == 40 and held == list(range(30, 70)) and c.plan.mw == 2 and c.G == 8
    # ---- pgen_table: ProgramGen's (column, |v|) keys against the slots of the pair table, which build_plan sizes from the triples.
    # a, b: exactly full (tab_find on a table without an empty slot); c: 84 keys for 64 slots; d: b with rows 0 and 1 sharing column 0 --
    # Triangle finds the quotient 6 / -2 = -3 in row 1 and records the SIGNED -2 in `multiples`: key 129 of 128 slots; e: two pairs, 66
    # keys -- the slots that twice the triples ask for are 64 again: the repeat must double the slots, not the estimate
    c = _cse_case(out, "a_64x1", "pgen_table", 64, [{i: 2 + i} for i in range(64)], costs=(0, 64), launches=1)
    assert (c.plan.cap, c.keys, c.plan.distinct) == (64, 64, 0)
    c = _cse_case(out, "b_64x2", "pgen_table", 128, [{2 * i: 2 + 2 * i, 2 * i + 1: 3 + 2 * i} for i in range(64)], costs=(64, 128), launches=1)
    assert (c.plan.cap, c.keys, c.plan.distinct, c.maxfreq) == (128, 128, 64, 1)
    rows = [{2 * i: 2 + 2 * i, 2 * i + 1: 3 + 2 * i} for i in range(20)] + [{40 + i: 50 + i} for i in range(44)]
    c = _cse_case(out, "c_20x2_44x1", "pgen_table", 84, rows, costs=(20, 84), launches=2)
    assert (c.plan.cap, c.keys, c.plan.distinct, c.maxfreq) == (64, 84, 20, 1) and wave_plan(c.m, c.n, c.rows, P, cap_scale=4).cap == 128
    rows = [{0: -2, 1: 5}, {0: 6, 2: 3}] + [{2 * i - 1: 5 + 2 * i, 2 * i: 6 + 2 * i} for i in range(2, 64)]
    c = _cse_case(out, "d_triangle", "pgen_table", 127, rows, launches=2)
    assert (c.plan.cap, c.keys, c.plan.distinct, c.maxfreq) == (128, 128, 64, 1) and wave_plan(c.m, c.n, c.rows, P, cap_scale=4).cap == 256
    q = c.rows[1][0] * pow(c.rows[0][0], -1, P) % P               # the couple (row 0, row 1) of column 0 and its quotient in row 1
    assert P - q == c.rows[1][2] == 3 and c.rows[0][0] == P - 2 and (0, P - 2) not in cse_pgen_keys(c.rows, P)
    rows = [{0: 2, 1: 3}, {2: 4, 3: 5}] + [{4 + i: 6 + i} for i in range(62)]
    c = _cse_case(out, "e_2x2_62x1", "pgen_table", 66, rows, costs=(2, 66), launches=2)
    assert (c.plan.cap, c.keys, c.plan.distinct) == (64, 66, 2) and wave_plan(c.m, c.n, c.rows, P, cap_scale=4).cap == 128
    # ---- pgen_shape: ProgramGen for general coefficients at full width
    for m in (63, 64):                                           # one row per lane in Triangle, the last lane idle / busy
        c = _cse_case(out, "gen%dx6" % m, "pgen_shape", *_dense(rng, m, 6, [1, -1, 2, 3, -2], 0.8), random=True)
        assert not c.plan.unit and c.plan.mw == 1
    # column 0 is non +-1 in all 64 rows, |v| = 2 .. 65 (nothing for FactorOutColumns); every odd row holds the quotient of its entry by the
    # row's above in a column of its own: Triangle fires on the couples (0, 1), (2, 3), ... 32 times in column 0, after the first one through
    # the `found` shortcut; every eighth pivot is negative (a new key of `multiples`)
    rows = []
    for i in range(64):
        a = (i + 2) * (-1 if i % 8 == 0 else 1)
        r = {0: a, 1 + i: 1}
        if i % 2:
            r[1 + i] = a * pow(rows[-1][0], -1, P) % P * (-1 if i % 4 == 1 else 1)
        rows.append(r)
    c = _cse_case(out, "triangle_64", "pgen_shape", 65, rows, couples=32)
    assert c.maxfreq == 1 and all(v % P not in (1, P - 1) for r in c.rows for j, v in r.items() if j == 0 or j % 2 == 0) and c.keys + 8 <= c.plan.cap
    # the never-reset `found`: after the couple (0, 1) only the first couple of what is left is looked at -- rows 2 and 3, which have no
    # quotient, and not rows 2 and 4, which have one: 6 multiplications, 5 for a scan that starts over
    rows = [{0: 2, 1: 1}, {0: 3, 2: 3 * pow(2, -1, P)}, {0: 5, 3: 1}, {0: 7, 4: 1}, {0: 11, 5: 11 * pow(5, -1, P)}]
    c = _cse_case(out, "triangle_found", "pgen_shape", 6, rows, costs=(5, 6))
    assert c.maxfreq == 1 and c.rows[4][5] * c.rows[2][0] % P == c.rows[4][0] and c.rows[3][4] == 1
    c = _cse_case(out, "factor_rows_2x64", "pgen_shape", *_factor_rows())
    assert c.maxfreq == 1 and c.maxlen == 64 and c.G == 1 and c.keys == 128
    # 22 blocks of two proportional rows over four columns of their own: three steps per block, each with a ratio that is no +-1 and a
    # column l1 of its own -- 66 multipliers when ProgramGen starts (the s0 += 64 loops over the multiplier list take two trips), and
    # 132 tied triples at the start.  The dense 30 x 8 matrix over 2 .. 39 has some 800 triples of which few repeat
    rows = []
    for b in range(22):
        w = _sample(rng, range(2, 40), 4)
        k = _pick(rng, [-1, 2, 3])
        rows += [{4 * b + j: w[j] for j in range(4)}, {4 * b + j: k * w[j] for j in range(4)}]
    c = _cse_case(out, "mult66_blocks", "pgen_shape", 88, rows, multipliers=66)
    assert (c.T, c.maxfreq) == (132, 2) and sum(len(r) - 1 for r in c.rows) >= 130
    c = _cse_case(out, "dense30x8", "pgen_shape", *_dense(rng, 30, 8, list(range(2, 40))))
    assert sum(len(r) - 1 for r in c.rows) >= 130
    # ---- moduli: rb from 2 to 31 bits (at 3 every residue is +-1), both branches of fmul, and the key of exactly 51 bits
    mu, mg = _dense(rng, 10, 7, [1, -1], 0.8), _dense(rng, 10, 7, [1, -1, 2, 3, 5, 6], 0.8)
    for p in CSE_MODULI:
        _cse_case(out, "unit_mod%d" % p, "moduli", *mu, p=p)
        c = _cse_case(out, "gen_mod%d" % p, "moduli", mg[0], [{j: (v if v % p else 1) for j, v in r.items()} for r in mg[1]], p=p)
        assert c.plan.unit == (p == 3)
    big = 2147483629
    one = [{1020: 1, 1021: -1}] + [{j: 1} for j in (0, 511, 1019, 1021, 1020, 7, 1000)]
    c = _cse_case(out, "key51_8x1022", "moduli", 1022, one, p=big)
    assert c.plan.NC == 1024 and 2 * _clog2(c.plan.NC) + _clog2(big) == 51
    pool = [0, 1, 500, 994, 995, 996, 997, 998, 999]               # the same width with steps: 22 new columns 1000 .. 1021 at the most
    c = _cse_case(out, "key51_8x1000", "moduli", 1000, _rows(rng, 1000, [7, 7, 7, 7, 6, 6, 6, 6], [1, -1], pool), p=big)
    assert c.plan.NC == 1024 and c.maxfreq >= 2
    c = _cse_case(out, "key53_8x1023", "moduli", 1023, [{1021: 1, 1022: -1}] + one[1:], p=big, refusal="PLO_E_CAPACITY")
    assert 1023 + 0 + 2 == 1025 and 2 * _clog2(1025) + _clog2(big) == 53
    assert all(not c.hbm or c.plan == "PLO_E_CAPACITY" for c in out)
    return out
