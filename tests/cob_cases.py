"""Inputs and references for the edge-shape tests of the change-of-basis enumeration (plo_cob.hip): no code under test here.

  * ref_range: one slice of an enumeration in plain Python on exact integers -- the rank of Cand with row := w by elimination
    mod p, zeros(TM^T w), zeros(w), the oracle's strict comparison, first winner in index order.  It makes 255 coefficients
    checkable: the C oracle has no range and cannot walk 255^4 candidates.
  * planted: a whole enumeration whose winner is known in O(C) (a target row w*, the columns of TM drawn in w*-perp).
  * coefficient lists with the good values LAST (.., 2, p-2, 1, p-1, 0): winners sit at l >= 64 and at large indices.
  * the case families of tests/test_gpu_cob_edges.py, with their references computed once per process and shared.
"""
import collections
import random

from plo_testlib import oracle_cob_search

P17, PA, PM = 131071, 2147483629, 2147483647
LDS_CAP = 160 * 1024                    # the library's cap on a workgroup's LDS
TAB_LIMIT = 72 * 1024                   # table kernel when its tables fit this

Case = collections.namedtuple("Case", "name n m TM Cand row off coeffs p")


def args(c):
    return (c.n, c.m, c.TM, c.Cand, c.row, c.off, c.coeffs, c.p)


# ---------------------------------------------------------------------------------------------- references
def _echelon(rows, n, p):
    """Row echelon basis of `rows` mod p by forward elimination: [(pivot column, row with a 1 there and 0 at the earlier pivots)]"""
    rows = [[x % p for x in r] for r in rows]
    basis = []
    for col in range(n):
        q = next((i for i, r in enumerate(rows) if r[col]), None)
        if q is None:
            continue
        r = rows.pop(q)
        iv = pow(r[col], -1, p)
        r = [x * iv % p for x in r]
        rows = [[(x - o[col] * y) % p for x, y in zip(o, r)] for o in rows]
        basis.append((col, r))
    return basis


def _in_span(basis, w, p):
    w = list(w)
    for col, r in basis:
        if w[col]:
            f = w[col]
            w = [(x - f * y) % p for x, y in zip(w, r)]
    return not any(w)


def ref_range(n, m, TM, Cand, row, off, coeffs, p, w0, w1, g0, gn):
    """The prefixes (i,j,k) g0 .. g0+gn-1, every l.  Returns (zeros_v, zeros_w, index, found) as oracle_cob_search does.
    rank(Cand with row := w) = rank(the other rows) + (w outside their span): the other rows are eliminated once."""
    C = len(coeffs)
    assert 0 <= g0 and g0 + gn <= C ** 3
    others = [Cand[i * n:(i + 1) * n] for i in range(n) if i != row]
    basis = _echelon(others, n, p)
    bv, bw, bidx, found = w0, w1, 0, 0
    for g in range(g0, g0 + gn):
        i, j, k = g // (C * C), g // C % C, g % C
        for l in range(C):
            w = [0] * n
            for t, x in enumerate((i, j, k, l)):
                if off + t < n:
                    w[off + t] = coeffs[x] % p
            if len(basis) + (0 if _in_span(basis, w, p) else 1) <= row:
                continue
            zv = sum(1 for c in range(m) if sum(w[q] * TM[q * m + c] for q in range(n) if w[q]) % p == 0)
            zw = sum(1 for x in w if not x)
            if zv > bv or (zv == bv and zw > bw):
                bv, bw, bidx, found = zv, zw, g * C + l, 1
    return bv, bw, bidx, found


def reduce_shards(results, n, w0, w1):
    """The reduction of tests/test_gpu_cob.py::test_cob_enumeration_sharded_by_prefix_equals_whole: largest score, smallest index"""
    best = None
    for res in results:
        if res[3]:
            key = (res[0] * (n + 1) + res[1], -res[2])
            if best is None or key > best[0]:
                best = (key, res)
    return best[1] if best else (w0, w1, 0, 0)


_whole = {}


def whole_ref(c, w0=-1, w1=-1):
    """The C oracle's result of the whole enumeration of a case, computed once per process"""
    key = (c.name, w0, w1)
    if key not in _whole:
        _whole[key] = oracle_cob_search(*args(c), w0, w1)
    return _whole[key]


_slices = {}


def slice_ref(c, w0, w1, g0, gn):
    key = (c.name, w0, w1, g0, gn)
    if key not in _slices:
        _slices[key] = ref_range(*args(c), w0, w1, g0, gn)
    return _slices[key]


# ---------------------------------------------------------------------------------------------- inputs
def usual_coeffs(C, p, zero=True):
    """0, 1, -1, 2, -2, ... : the order of the existing tests (good values first)"""
    out = [0] if zero else []
    k = 1
    while len(out) < C:
        out.append(k % p)
        if len(out) < C:
            out.append((p - k) % p)
        k += 1
    return out[:C]


def good_last(C, p, zero=True):
    """the same values with the good ones last: [.., 2, p-2, 1, p-1, 0]"""
    u = usual_coeffs(C, p, zero)
    return _pairs_reversed(u[1:]) + [0] if zero else _pairs_reversed(u)


def _pairs_reversed(u):
    """[1, p-1, 2, p-2, 3] -> [3, 2, p-2, 1, p-1]"""
    pairs = [u[k:k + 2] for k in range(0, len(u), 2)]
    return [x for pr in reversed(pairs) for x in pr]


def chosen_rows(rng, n, row, p, kind):
    """Cand with rows 0..row-1 chosen: "unit" (1 on the diagonal, random to its right: independent), "random" (maybe dependent),
    "dependent" (the last chosen row repeats the first, or is zero when there is only one)"""
    Cand = [0] * (n * n)
    for i in range(row):
        for j in range(n):
            if kind == "unit":
                Cand[i * n + j] = 1 if j == i else (rng.choice([0, 1, p - 1, 2]) % p if j > i else 0)
            else:
                Cand[i * n + j] = rng.choice([0, 1, p - 1, 2]) % p
    if kind == "dependent" and row:
        for j in range(n):
            Cand[(row - 1) * n + j] = Cand[j] if row > 1 else 0
    return Cand


def rand_case(name, seed, C, n, m, row, p, off=None, coeffs=None, chosen="unit", dense_last=False, wide=False):
    """dense_last: row off+3 of TM is dense with large values, so that the winner leaves it out (w[3] = 0, the LAST coefficient of
    a good_last list: l = C-1).  wide: entries of TM from the whole of Z_p."""
    rng = random.Random(seed)
    off = (row // 4) * 4 if off is None else off
    vals = [0, 0, 1, p - 1, 2, 3]
    TM = [(rng.randrange(p) if wide and rng.random() < 0.5 else rng.choice(vals) % p) for _ in range(n * m)]
    if dense_last and off + 3 < n:
        for c in range(m):
            TM[(off + 3) * m + c] = rng.randrange(p // 3, p - 3)
    Cand = chosen_rows(rng, n, row, p, chosen)
    return Case(name, n, m, TM, Cand, row, off, list(coeffs) if coeffs is not None else good_last(C, p), p)


def planted(C, p, idx4, row, seed=0):
    """n = 4, block 0, m = 4, C distinct non-zero coefficients (good values last), target w* = coefficients at idx4; the columns of
    TM are random in w*-perp with the 4 x m block of rank 3, so zeros(TM^T w) = m exactly for the multiples of w*.  Returns
    (case, expected): the winner is the multiple s*w* whose four entries are coefficients, independent of the chosen row for
    row = 1, with the largest zeros(w), then the smallest index -- found in O(C)."""
    assert row in (0, 1)
    rng = random.Random(seed * 1000003 + C * 7 + row)
    n = m = 4
    coeffs = good_last(C, p, zero=False)
    assert len(set(coeffs)) == C and 0 not in coeffs
    ws = [coeffs[x] for x in idx4]
    while True:
        cols = []
        for _ in range(m):
            u = [rng.randrange(p) for _ in range(3)]
            u.append(-(u[0] * ws[0] + u[1] * ws[1] + u[2] * ws[2]) * pow(ws[3], -1, p) % p)
            cols.append(u)
        if len(_echelon(cols, 4, p)) == 3:
            break
    TM = [cols[c][q] for q in range(n) for c in range(m)]
    Cand = [0] * (n * n)
    if row == 1:
        while True:
            r0 = [rng.choice([0, 1, p - 1, 2]) for _ in range(n)]
            if len(_echelon([r0, ws], 4, p)) == 2:
                break
        Cand[:n] = r0
    where = {v: x for x, v in enumerate(coeffs)}
    iv, best = pow(ws[0], -1, p), None
    for cx in coeffs:
        s = cx * iv % p
        w = [s * x % p for x in ws]
        if not all(x in where for x in w):
            continue
        if row == 1 and len(_echelon([Cand[:n], w], 4, p)) < 2:
            continue
        ids = [where[x] for x in w]
        key = (sum(1 for x in w if not x), -(((ids[0] * C + ids[1]) * C + ids[2]) * C + ids[3]))
        if best is None or key > best:
            best = key
    name = "planted-C%d-p%d-r%d-%s" % (C, p, row, "_".join(map(str, idx4)))
    return Case(name, n, m, TM, Cand, row, 0, coeffs, p), (m, best[0], -best[1], 1)


# ---------------------------------------------------------------------------------------------- case families
def wave_width_cases():
    """(a) whole enumerations across the wave width, against the C oracle: every value of C in {63,64,65}, n in {4,5}, m in {4,6},
    row in {0,1} occurs, and one n = 6 case in the last block (fb = 2).  ~2.5 s of oracle each: not the full cross."""
    mk = lambda C, n, m, row, **kw: rand_case("wave-C%d-n%d-m%d-r%d" % (C, n, m, row), 100 + C + 7 * n + 3 * m + row, C, n, m, row, P17, dense_last=True, **kw)
    return [mk(65, 4, 4, 0), mk(65, 4, 4, 1), mk(65, 5, 6, 1),
            mk(64, 4, 4, 0), mk(64, 4, 4, 1), mk(64, 5, 6, 0),
            mk(63, 5, 4, 1), mk(63, 4, 6, 0),
            mk(63, 6, 4, 4, off=4)]


SLICE_N = {1: (0, 0), 4: (0, 1), 5: (4, 4), 6: (4, 5), 7: (4, 4)}            # n -> (off, row): fb = 1, 4, 1, 2, 3


def slice_cases():
    """(b) C in {65,128,129,255} x n in {1,4,5,6,7} (the last block: fb = 1, 2, 3)"""
    out = []
    for C in (65, 128, 129, 255):
        for n, (off, row) in SLICE_N.items():
            p = [P17, PA, PM, 101][(C + n) % 4]
            out.append(rand_case("slice-C%d-n%d" % (C, n), 7 * C + n, C, n, 3 + (C + n) % 5, row, p, off=off, wide=True))
    return out


def slices_of(C):
    """(first_group, ngroups): the first 3, the last 3, 4 across an i boundary, counts 1, 3, 5, 9, and none"""
    G = C ** 3
    return [(0, 3), (G - 3, 3), (C * C - 2, 4), (G // 2 + 11, 1), (G // 3, 3), (2 * C * C + C - 3, 5), (G - C * C - 4, 9), (G // 5, 0), (G, 0)]


def slice_thresholds(c, k):
    """thresholds for the k-th slice of a case: mostly none, some that a slice's winner may or may not beat"""
    return [(-1, -1), (-1, -1), (0, -1), (-1, -1), (c.m // 2, 0), (-1, 3), (1, c.n), (-1, -1), (2, 1)][k]


def planted_cases():
    """(c): (kernel, C, p, row, target indices) with l = C-1 and with i = C-1"""
    out = []
    for generic, C in ((False, 255), (True, 129)):
        for row, p, idx4 in ((0, P17, (3, C // 2, 70, C - 1)), (1, PA, (C - 1, 5, C - 2, 66)), (1, P17, (C - 1, C - 1, 1, C - 1)), (0, PA, (C - 2, 0, 64, C - 1))):
            out.append((generic,) + planted(C, p, idx4, row))
    return out


def qn_row0(n, off):
    """columns of the nullspace block when no row is chosen yet: the unit vectors of the block"""
    return min(4, n - off)


def lds_model(C, m, qn, generic):
    """(bytes, table kernel?) of one enumeration: the table kernel's [4][C][m|1] and [4][C][max(qn,1)|1] words when they fit 72 KiB,
    else the generic kernel's 4 x m block, 4 x qn block and C coefficients"""
    tab = 4 * C * ((m | 1) + (max(qn, 1) | 1)) * 4
    if tab <= TAB_LIMIT and not generic:
        return tab, True
    return (4 * m + 4 * qn + C) * 4, False


def switch_cases():
    """(d) C = 7, n = 4, row 0, m = 652, 653 (tables: 7*(653+5) = 4606 <= 4608) and 654 (7*(655+5) = 4620: generic)"""
    return [rand_case("switch-m%d" % m, 900 + m, 7, 4, m, 0, P17, coeffs=usual_coeffs(7, P17)) for m in (652, 653, 654)]


def generic_limit_m(C, qn):
    """the largest m whose generic-kernel LDS (4m + 4qn + C words) fits the cap"""
    return (LDS_CAP // 4 - 4 * qn - C) // 4


def threshold_cases():
    """(e) one case whose winner has zeros(w) >= 1, one whose coefficients lack 0 (n = 4: zeros(w) == 0)"""
    a = rand_case("thr-zw", 41, 9, 5, 7, 1, P17, coeffs=usual_coeffs(9, P17))
    b = rand_case("thr-nozero", 42, 8, 4, 6, 1, PA, coeffs=usual_coeffs(8, PA, zero=False))
    return [a, b]


def thresholds_around(zv, zw, n):
    """[(w0, w1, found expected)] around a winner (zv, zw); the last two: a w1 beyond n stays in its own digit"""
    out = [(zv, zw - 1, 1), (zv, zw, 0), (zv - 1, n, 1), (zv + 1, -1, 0), (-1, 3, 1), (zv, n + 1, 0), (zv - 1, n + 1, 1), (zv - 1, 1 << 20, 1)]
    if zw == 0:
        assert (zv, -1, 1) in out               # (zv*, zw*-1) is (zv*, -1)
    return out


def moduli_cases():
    """(f) small moduli whose coefficient values collide, operands all p-1, coefficients >= p"""
    out = []
    for p in (3, 5):
        five = [0, 1, p - 1, 2 % p, (p - 2) % p]
        for n, row in ((4, 0), (4, 2), (6, 1)):
            out.append(rand_case("mod%d-n%d-r%d" % (p, n, row), 50 + p + n + row, 5, n, 9, row, p, coeffs=five))
    for p in (PM, PA):
        for n, row in ((4, 0), (5, 1), (5, 0)):
            c = rand_case("max%d-n%d-r%d" % (p, n, row), 1, 5, n, 6, row, p, coeffs=[p - 1] * 5)
            Cand = [0] * (n * n)
            Cand[:row * n] = [p - 1] * (row * n)
            out.append(c._replace(TM=[p - 1] * (n * c.m), Cand=Cand))
    for p in (PM, P17, 7):
        for n, row in ((4, 0), (5, 1)):
            out.append(rand_case("multiples%d-n%d-r%d" % (p, n, row), 60 + n, 6, n, 8, row, p, coeffs=[1, p, p - 1, 2 * p, 2, p + 1]))
    return out


def batch_sets():
    """(g) [(name, n, m, row, off, [case, ...])]: four problems with C = (65, 3, 64, 1) around the row-1 inputs of (a); the same with
    the second problem's chosen row dependent; and a batch at the m = 654 of (d) in which the C = 7 problem alone does not fit the
    tables."""
    W = {c.name: c for c in wave_width_cases()}
    c65, c64 = W["wave-C65-n4-m4-r1"], W["wave-C64-n4-m4-r1"]
    c3 = rand_case("batch-C3", 71, 3, 4, 4, 1, PA)
    c1 = rand_case("batch-C1", 72, 1, 4, 4, 1, 101, coeffs=[1])
    d3 = rand_case("batch-C3-dependent", 73, 3, 4, 4, 1, PA, chosen="dependent")
    sw = switch_cases()[2]
    s3 = rand_case("batch-m654-C3", 74, 3, 4, sw.m, 0, PM)
    s5 = rand_case("batch-m654-C5", 75, 5, 4, sw.m, 0, 101)
    s1 = rand_case("batch-m654-C1", 76, 1, 4, sw.m, 0, P17, coeffs=[P17 - 1])
    return [("unequal", 4, 4, 1, 0, [c65, c3, c64, c1]), ("dependent", 4, 4, 1, 0, [c65, d3, c64, c1]), ("fallback", 4, sw.m, 0, 0, [s3, sw, s5, s1])]
