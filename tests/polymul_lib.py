"""Helpers of the polynomial-multiplication tests (bin/PMchecker, plo_polymul_*): an oracle that shares no code with the product,
and generators of triples that are correct by construction.

A matrix is (rows, columns, {(i, j): Fraction}) as plo_testlib.read_sms returns it; a triple is (L, R, P) with L r x na, R r x nb,
P nc x r.  The pair (i, j) has the sums S[z] = sum_t L[t][i] R[t][j] P[z][t] (z < nc) and the defect polynomial
D_ij = sum_z S[z] X^z - X^(i+j).  With Z = max(nc, na + nb - 1): without f the width is w = Z and equation e = (i nb + j) w + c asks
for coefficient c of D_ij to vanish; with f of degree d the width is d and it asks for coefficient c of D_ij mod f to vanish.

The oracle works on dense lists of Python integers modulo q, or of Fractions over Q (q = 0), and takes remainders by plain long
division by f: it has no table of X^z mod f, so a wrong table cannot agree with it.  It returns (violated, first, value,
expected): the number of violated equations, the smallest e (None when there is none), and there the coefficient of
(sum_z S[z] X^z) mod f and that of X^(i+j) mod f."""
import math
import os
from fractions import Fraction

from plo_testlib import DATA, read_sms

P31 = 2147483629


def load(name):
    return tuple(read_sms(os.path.join(DATA, "%s_%s.sms" % (name, x))) for x in "LRP")


def files(name):
    return [os.path.join(DATA, "%s_%s.sms" % (name, x)) for x in "LRP"]


def shape(T):
    """(na, nb, nc, Z)"""
    na, nb, nc = T[0][1], T[1][1], T[2][0]
    return na, nb, nc, max(nc, na + nb - 1)


def width(T, f=None):
    return len(f) - 1 if f else shape(T)[3]


def residue(v, q):
    v = Fraction(v)
    return v.numerator % q * pow(v.denominator % q, -1, q) % q


def conv(v, q):
    return Fraction(v) if q == 0 else residue(v, q)


def poly(text):
    """A polynomial of the tests from its coefficients as text, constant term first: poly("1 -1 0 0 0 1") is 1 - X + X^5"""
    return [Fraction(x) for x in text.split()]


def poly_text(f, X="X"):
    """The text that -P takes, lowest term first: 1-X+X^5"""
    out = ""
    for e, c in enumerate(f):
        if c == 0:
            continue
        a = abs(c)
        term = (str(a) if a != 1 or e == 0 else "") + (("*" if a != 1 else "") + X + ("^%d" % e if e > 1 else "") if e else "")
        out += ("-" if c < 0 else "+" if out else "") + term
    return out


def rem(a, f, q):
    """a mod f by long division, a and f dense coefficient lists (constant term first) over Z/qZ or Q; len(f) - 1 coefficients"""
    d = len(f) - 1
    a = list(a) + [0] * max(0, d - len(a))
    inv = 1 / f[d] if q == 0 else pow(f[d], -1, q)
    for k in range(len(a) - 1, d - 1, -1):
        c = a[k] * inv
        if q:
            c %= q
        if c:
            for t in range(d + 1):
                a[k - d + t] = (a[k - d + t] - c * f[t]) if q == 0 else (a[k - d + t] - c * f[t]) % q
        assert a[k] == 0
    return a[:d]


def by_product(T, q):
    """per product t: the entries of row t of L, of row t of R and of column t of P, as lists of (index, value) over the field"""
    r = T[0][0]
    rows = [([], [], []) for _ in range(r)]
    for which, M in enumerate(T):
        for (i, j), v in M[2].items():
            t, x = (j, i) if which == 2 else (i, j)
            c = conv(v, q)
            if c:
                rows[t][which].append((x, c))
    return rows


def sums(T, q):
    """S[i][j] = the nc sums of the pair, over Z/qZ or Q"""
    na, nb, nc, _ = shape(T)
    S = [[[0] * nc for _ in range(nb)] for _ in range(na)]
    for ls, rs, ps in by_product(T, q):
        for i, lv in ls:
            for j, rv in rs:
                lr = lv * rv
                row = S[i][j]
                for z, pv in ps:
                    row[z] += lr * pv
    if q:
        for i in range(na):
            for j in range(nb):
                S[i][j] = [x % q for x in S[i][j]]
    return S


def field_poly(f, q):
    return [conv(c, q) for c in f] if f else None


def pair_values(S_ij, i, j, Z, fq, q):
    """(found, expected) of one pair, each a list of w values"""
    got = list(S_ij) + [0] * (Z - len(S_ij))
    want = [0] * Z
    want[i + j] = 1
    if fq is None:
        return got, want
    d = len(fq) - 1
    got, want = rem(got, fq, q), rem(want, fq, q)
    diff = rem([(a - b) if q == 0 else (a - b) % q for a, b in zip(list(S_ij) + [0] * (Z - len(S_ij)), [int(z == i + j) for z in range(Z)])], fq, q)
    assert diff == [(a - b) if q == 0 else (a - b) % q for a, b in zip(got, want)] and len(got) == d        # D_ij mod f, taken at once
    return got, want


def oracle(T, q=0, f=None, pair0=0, pair1=None):
    """(violated, first, value, expected) among the pairs [pair0, pair1)"""
    na, nb, nc, Z = shape(T)
    fq = field_poly(f, q)
    S = sums(T, q)
    pair1 = na * nb if pair1 is None else pair1
    cnt, first = 0, None
    for pair in range(pair0, pair1):
        i, j = divmod(pair, nb)
        got, want = pair_values(S[i][j], i, j, Z, fq, q)
        for c, (a, b) in enumerate(zip(got, want)):
            if a != b:
                cnt += 1
                if first is None:
                    first = (pair * len(got) + c, a, b)
    return (cnt, None, None, None) if first is None else (cnt,) + first


def bits(v):
    return abs(int(v)).bit_length()


def primitive(f):
    """f over the integers, primitive"""
    l = 1
    for c in f:
        l = l * c.denominator // math.gcd(l, c.denominator)
    z = [int(c * l) for c in f]
    g = 0
    for c in z:
        g = math.gcd(g, c)
    return [c // g for c in z]


def cleared_defect_bits(T, f=None):
    """The bit length of the largest coefficient that the certificate has to bound, over Q: D D_ij, D the product of the lcms of
    the denominators of L, R and P, and with f its pseudo-remainder by the primitive integer f in Z - d steps"""
    na, nb, nc, Z = shape(T)
    D = 1
    for M in T:
        l = 1
        for v in M[2].values():
            l = l * v.denominator // math.gcd(l, v.denominator)
        D *= l
    S = sums(T, 0)
    fz = primitive(f) if f else None
    worst = 0
    for i in range(na):
        for j in range(nb):
            a = [D * x for x in S[i][j]] + [0] * (Z - nc)
            a[i + j] -= D
            assert all(x.denominator == 1 for x in a)
            a = [int(x) for x in a]
            worst = max([worst] + [bits(x) for x in a])
            if fz and len(fz) - 1 < Z:
                d = len(fz) - 1
                for k in range(Z - 1, d - 1, -1):
                    top = a[k]
                    a = [fz[d] * x for x in a]
                    for t in range(d + 1):
                        a[k - d + t] -= top * fz[t]
                    assert a[k] == 0
                    worst = max([worst] + [bits(x) for x in a])
    return worst


def certificate(T, f=None):
    """(beta, j) as DESIGN.md 2.13 states them"""
    na, nb, nc, Z = shape(T)
    beta = bits(T[0][0]) + 2
    for M in T:
        beta += max([bits(v.numerator) for v in M[2].values()] or [0])
        beta += sum(bits(d) for d in {v.denominator for v in M[2].values()} if d > 1)
    if f:
        fz = primitive(f)
        d = len(fz) - 1
        if d < Z:
            beta += (Z - d) * bits(abs(fz[d]) + max(abs(c) for c in fz))
    return beta, -(-beta // 30)


# ----------------------------------------------------------------------------- triples that are correct by construction
def schoolbook(na, nb):
    """r = na nb, one product per (i, j), nc = na + nb - 1"""
    L, R, P = {}, {}, {}
    for i in range(na):
        for j in range(nb):
            t = i * nb + j
            L[(t, i)] = Fraction(1); R[(t, j)] = Fraction(1); P[(i + j, t)] = Fraction(1)
    return (na * nb, na, L), (na * nb, nb, R), (na + nb - 1, na * nb, P)


def power_mod(e, f):
    """X^e mod f over Q by e multiplications by X (no division of polynomials: another way than the oracle's)"""
    d = len(f) - 1
    v = [Fraction(0)] * d
    if e < d:
        v[e] = Fraction(1)
        return v
    v = power_mod(e - 1, f)
    top = v[d - 1]
    return [(v[c - 1] if c else 0) - top * f[c] / f[d] for c in range(d)]


def schoolbook_folded(na, nb, f):
    """schoolbook with P folded by f beforehand: nc = d, column t of P is X^(i+j) mod f"""
    L, R, _ = schoolbook(na, nb)
    d = len(f) - 1
    P = {}
    for i in range(na):
        for j in range(nb):
            for c, v in enumerate(power_mod(i + j, f)):
                if v:
                    P[(c, i * nb + j)] = v
    return L, R, (d, na * nb, P)


def karatsuba(k):
    """nested Karatsuba of depth k: 2^k coefficients each, 3^k products, nc = 2^(k+1) - 1"""
    if k == 0:
        one = {(0, 0): Fraction(1)}
        return (1, 1, dict(one)), (1, 1, dict(one)), (1, 1, dict(one))
    A = karatsuba(k - 1)
    r, n = A[0][0], A[0][1]
    halves = []
    for M in A[:2]:                                                # rows [M | 0], [0 | M], [M | M]
        E = {}
        for (t, x), v in M[2].items():
            E[(t, x)] = v; E[(r + t, n + x)] = v; E[(2 * r + t, x)] = v; E[(2 * r + t, n + x)] = v
        halves.append((3 * r, 2 * n, E))
    P = {}

    def add(z, t, v):
        P[(z, t)] = P.get((z, t), 0) + v

    for (z, t), v in A[2][2].items():                              # c = p0 + X^n (p2 - p0 - p1) + X^2n p1
        add(z, t, v); add(z + n, t, -v)
        add(z + 2 * n, r + t, v); add(z + n, r + t, -v)
        add(z + n, 2 * r + t, v)
    return halves[0], halves[1], (4 * n - 1, 3 * r, {k_: v for k_, v in P.items() if v})


def scaled(T, scales):
    """product t scaled by scales[t] in L and by its inverse in P"""
    L, R, P = T
    return ((L[0], L[1], {(t, x): v * scales[t] for (t, x), v in L[2].items()}), R,
            (P[0], P[1], {(z, t): v / scales[t] for (z, t), v in P[2].items()}))


def grown(T, extra):
    """the triple with `extra` more products, all empty"""
    L, R, P = T
    return (L[0] + extra, L[1], dict(L[2])), (R[0] + extra, R[1], dict(R[2])), (P[0], P[1] + extra, dict(P[2]))


def with_null_products(T, count, i, j, rng, lo=1, hi=9):
    """`count` products with random entries in column i of L and column j of R and a zero column of P: the two columns grow by
    `count` entries that share their t, the bilinear map stays"""
    r = T[0][0]
    L, R, P = grown(T, count)
    for t in range(r, r + count):
        L[2][(t, i)] = Fraction(rng.randrange(lo, hi)); R[2][(t, j)] = Fraction(rng.randrange(lo, hi))
    return L, R, P


def with_cancelling_pair(T, length, i, j, rng, lo=1, hi=9):
    """two products with the same rows in L and R (one entry each, in columns i and j) and columns v and -v of P, v with
    `length` entries: rows of P^T of that length, the bilinear map stays"""
    r = T[0][0]
    L, R, P = grown(T, 2)
    assert length <= P[0]
    a, b = Fraction(rng.randrange(lo, hi)), Fraction(rng.randrange(lo, hi))
    for t in (r, r + 1):
        L[2][(t, i)] = a; R[2][(t, j)] = b
    for z in range(length):
        v = Fraction(rng.randrange(lo, hi))
        P[2][(z, r)] = v; P[2][(z, r + 1)] = -v
    return L, R, P


def with_full_cancelling_pairs(T, pairs, rng, hi=1000):
    """`pairs` cancelling pairs of products whose rows of L and R and columns of P are full: a dense input (DESIGN.md 2.13 measures one)"""
    r = T[0][0]
    L, R, P = grown(T, 2 * pairs)
    for t in range(r, r + 2 * pairs, 2):
        for x in range(L[1]):
            a = Fraction(rng.randrange(1, hi))
            L[2][(t, x)] = L[2][(t + 1, x)] = a
        for y in range(R[1]):
            b = Fraction(rng.randrange(1, hi))
            R[2][(t, y)] = R[2][(t + 1, y)] = b
        for z in range(P[0]):
            v = Fraction(rng.randrange(1, hi))
            P[2][(z, t)] = v; P[2][(z, t + 1)] = -v
    return L, R, P


def with_rows(T, nc):
    """P with nc rows: more rows are zero rows, fewer cut the top coefficients off"""
    L, R, P = T
    return L, R, (nc, P[1], {(z, t): v for (z, t), v in P[2].items() if z < nc})


def changed(T, which, i, j, value):
    """the triple with one entry of L (0), R (1) or P (2) set to `value` (0 removes it)"""
    mats = [(a, b, dict(ent)) for a, b, ent in T]
    if value == 0:
        mats[which][2].pop((i, j), None)
    else:
        mats[which][2][(i, j)] = Fraction(value)
    return tuple(mats)


def all_entries(T, value):
    """every entry replaced by `value`"""
    return tuple((a, b, {ij: Fraction(value) for ij in ent}) for a, b, ent in T)


# ----------------------------------------------------------------------------- to the product
def csr(M):
    """(rows, columns, rowptr, col, num, den) for plinopt_amd.PolyMulPlan"""
    rows, cols, ent = M
    rp, col, num, den = [0], [], [], []
    by_row = {}
    for (i, j), v in ent.items():
        by_row.setdefault(i, []).append((j, v))
    for i in range(rows):
        for j, v in sorted(by_row.get(i, [])):
            col.append(j); num.append(v.numerator); den.append(v.denominator)
        rp.append(len(col))
    return rows, cols, rp, col, num, den


def plan_poly(f):
    return [(c.numerator, c.denominator) for c in f] if f else None


def write_sms(path, M):
    rows, cols, ent = M
    with open(path, "w") as fh:
        fh.write("%d %d R\n" % (rows, cols))
        for (i, j), v in sorted(ent.items()):
            fh.write("%d %d %s\n" % (i + 1, j + 1, v))
        fh.write("0 0 0\n")


def write_triple(tmp, T, stem="t"):
    names = [os.path.join(str(tmp), "%s_%s.sms" % (stem, x)) for x in "LRP"]
    for p, M in zip(names, T):
        write_sms(p, M)
    return names


# (fixture, q, polynomial or None, violated equations): the lines of the issue's table, 0 = correct
F243 = poly("1 -1 0 0 0 1")
F243M = poly("-1 0 -1 -1 1 1")
F32S = poly("1 0 1 0 0 1")
F32M = poly("1 1 1 0 1 1")
F81 = poly("1 1 1 1 1")
X3 = poly("0 0 0 1")
CASES = [
    ("4o4o8_Toom5", 0, None, 0), ("4o4o8_Toom5", 131071, None, 0), ("4o4o8_Toom5", P31, None, 0),
    ("4o4o8_Montgomery-13", 0, None, 0), ("4o4o8_Montgomery-13", 7, None, 0),
    ("1o1o2_3_Karatsuba", 0, None, 0), ("2o2o4_Toom3", 0, None, 0), ("2o2o4_5_Toom3", 0, None, 0), ("3o3o6_Toom4", 0, None, 0),
    ("4o4o4_F243-11-44", 3, F243, 0), ("4o4o4_F243-Montgomery-13-42", 3, F243M, 0),
    ("4o4o4_F32_Standard", 2, F32S, 0), ("4o4o4_F32_Montgomery", 2, F32M, 0), ("3o3o3_F81-Karatsuba-9-21", 3, F81, 0),
    ("2o2o2_5_shortproduct", 0, X3, 0), ("4o4o8_Toom5", 0, F243, 0),
    ("2o2o2_5_shortproduct", 0, None, 3), ("2o2o2_4_partSP", 0, X3, 2), ("4o4o4_F243-Montgomery-13-42", 0, F243M, 33),
    ("3o3o3_S81_8_22", 3, F81, 30), ("4o4o4_S243_10-43", 3, F243, 43), ("4o4o4_S32_13_#2", 2, F32S, 53),
]


def case_id(case):
    name, q, f, _ = case
    return "%s-%s-%s" % (name, "Q" if q == 0 else q, poly_text(f) if f else "none")
