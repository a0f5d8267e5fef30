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
