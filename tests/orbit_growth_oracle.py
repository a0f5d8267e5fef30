"""Literal oracle of the growth-factor measure of the orbit search (bin/orbiter -g, PLO_ORBIT_GROWTH of include/plinopt_hip.h)
and of bin/growthfactor (reference src/growthfactor.cpp).

The measure: the transformed triple (Lj, Rg, hP) comes from tests/orbit_oracle.py / tests/orbit_action_oracle.py as exact
fractions (dense Kronecker products, Gauss-Jordan inverses).  Row g of the 3r rows (the rows of L, of R, the columns of P) is
scaled by c_g, the lcm of the denominators of the INPUT row, as the plan does; S_g is the sum of the squares of the scaled
outputs as a Python integer; then, in IEEE doubles with one rounding per operation (Python's float, math.sqrt),
    n_g = sqrt(float(S_g)) / float(c_g),      cost = sum_i (n_i * n_{r+i}) * n_{2r+i}   from 0.0, i increasing.
float(int) rounds to nearest: exact below 2^53, one rounding beyond, as the host tool does for the inputs the device refuses.

`growthfactor_text` restates the eleven numbers of src/growthfactor.cpp:185-231 and their text."""
import math
import struct
from fractions import Fraction

import numpy as np

import orbit_action_oracle as A
import orbit_oracle as O

BASE_SEED = O.BASE_SEED


def bits(x):
    """the 64-bit pattern of a double"""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _lists(M):
    return M.tolist() if isinstance(M, np.ndarray) else M


def _scale(row):
    c = 1
    for x in row:
        d = Fraction(x).denominator
        c = c * d // math.gcd(c, d)
    return c


def norms(in_rows, out_rows):
    """n_g of every row: in_rows give the scales, out_rows the transformed entries"""
    res = []
    for src, row in zip(in_rows, out_rows):
        c = _scale(src)
        S = 0
        for x in row:
            v = Fraction(x) * c
            assert v.denominator == 1, "an output is no multiple of 1/scale"
            S += int(v) ** 2
        res.append(math.sqrt(float(S)) / float(c))
    return res


def growth(mats, prods):
    """(cost, nnz, nno) of the transformed triple prods = (Lj, Rg, hP) of the input mats = (L, R, P)"""
    L, R, P = [_lists(M) for M in mats]
    Lj, Rg, hP = [_lists(M) for M in prods]
    nl, nr, np_ = norms(L, Lj), norms(R, Rg), norms(O.transpose(P), O.transpose(hP))
    cost = 0.0
    for i in range(len(L)):
        lr = nl[i] * nr[i]
        t = lr * np_[i]
        cost = cost + t
    _, nnz, nno = O.counts(Lj, Rg, hP)
    return cost, nnz, nno


def cost3(mats, mkn, seed, action=A.TRIANGULAR):
    return growth(mats, A.products(mats, mkn, seed, action))


def key(c, seed):
    """the search's order: (bits of the cost, nnz, nno, seed)"""
    return bits(c[0]), c[1], c[2], seed


# ---------------------------------------------------------------------------------------------- bin/growthfactor
def _div(a, b):
    """IEEE division as C++ does it (Python raises on a zero divisor); 0/0 is the default NaN of x86, whose sign bit is set"""
    if b == 0.0:
        if a == 0.0 or math.isnan(a):
            return -math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _log(x):
    if math.isnan(x) or x < 0:
        return -math.nan
    if x == 0.0:
        return -math.inf
    return math.log(x) if x != math.inf else math.inf


def _fixed(x):
    """std::fixed, precision 6"""
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return "%.6f" % x


def _entries(M):
    """per row the non-zero entries (column, double(num)/double(den)) in column order"""
    return [[(j, float(Fraction(x).numerator) / float(Fraction(x).denominator)) for j, x in enumerate(row) if x != 0] for row in _lists(M)]


def _norm1(v):
    s = 0.0
    for x in v:
        s += abs(x)
    return s


def _norm2(v):
    s = 0.0
    for x in v:
        s += x * x
    return math.sqrt(s)


def growth_numbers(mats, mkn):
    """[(label, value)] of the eleven `##` lines"""
    L, R, P = [_entries(M) for M in mats]
    m, k, n = mkn
    r = len(L)
    Pt = [[] for _ in range(r)]
    for j, row in enumerate(P):
        for i, v in row:
            Pt[i].append((j, v))

    def gp(norm):
        lr = [norm([v for _, v in L[i]]) * norm([v for _, v in R[i]]) for i in range(r)]
        out = []
        for row in P:
            s = 0.0
            for i, v in row:
                s += lr[i] * abs(v)
            out.append(s)
        return out

    gpinf, gp2 = gp(_norm1), gp(_norm2)
    ginfinf, ginf2, g2inf, g22 = max(gpinf), max(gp2), _norm2(gpinf), _norm2(gp2)
    g2 = 0.0
    for i in range(r):
        g2 += _norm2([v for _, v in L[i]]) * _norm2([v for _, v in R[i]]) * _norm2([v for _, v in Pt[i]])
    n0 = [float(len(L[i]) * len(R[i])) for i in range(r)]
    q0 = max(max([0.0] + [n0[i] for i, _ in row]) + float(len(row)) for row in P)

    def qk(gamma, kk):
        return _div(q0 * gamma, abs(gamma - kk))

    sq = math.sqrt(float(k))
    return [("Ginfinf:\t", ginfinf), ("Ginf2:\t", ginf2), ("G2inf:\t", g2inf), ("G22:\t\t", g22), ("G2:\t\t", g2), ("Q0:\t\t", q0),
            ("Qkinfinf:\t", qk(ginfinf, float(k))), ("Q1inf2:\t", qk(ginf2, 1.0)), ("Qk12inf:\t", qk(g2inf, 1.0)), ("Qk2inf:\t", qk(g2inf, sq * sq * sq)), ("Q122:\t", qk(g22, 1.0))]


def growthfactor_text(mats, mkn):
    m, k, n = mkn
    out = "# Norms of %dx%dx%d Matrix-Multiplication:\n#  \t\tGamma \t\tlog_%d\n" % (m, k, n, k)
    for label, v in growth_numbers(mats, mkn):
        out += "## %s%s\t%s\n" % (label, _fixed(v), _fixed(_div(_log(v), math.log(float(k)))))
    return out
