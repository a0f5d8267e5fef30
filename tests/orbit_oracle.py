"""Literal oracle of one candidate of the De Groote orbit search (bin/orbiter, reference src/orbiter.cpp:272-324), with
fractions.Fraction: dense U, V, W drawn from the candidate's stream (include/plinopt_hip.h, PLO_ORBIT_*), their inverses
by Gauss-Jordan, the Kronecker products J = U^-1 (x) V, G = (V^-1)^T (x) W, H = U (x) W^-1 formed entry by entry as
`Tensor` does (include/plinopt_library.inl:209-222), and the dense products L.J, R.G, H.P.  Over Z_mod the rational
products are reduced at the end.  It shares nothing with the kernel's sandwich and triangular shortcuts.

Counts of a candidate: nnz (non-zero entries of the three products), nno (those that are not +-1) and the canonical rows
(rows of L.J and R.G, columns of H.P, with exactly one non-zero).  cost = nnz for the density measure (-s, and every run
over Z_mod); L.m + R.m + P.n - canonical rows for -c."""
from fractions import Fraction

import numpy as np

from plo_testlib import read_sms

_M64 = (1 << 64) - 1
BASE_SEED = _M64
DENSITY, CANONICAL = 0, 2


class CandRng:
    """include/plinopt_hip.h: splitmix64 of the seed -> GivRandom's LCG (x <- 950706376 x mod 2^31-1)."""

    def __init__(self, seed):
        x = (seed + 0x9E3779B97F4A7C15) & _M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
        x ^= x >> 31
        self.s = 1 + x % 2147483646

    def next(self):
        self.s = (950706376 * self.s) % 2147483647
        return self.s


def zoi_matrix(rng, s):
    """The stream's s x s matrix: Fisher-Yates P, then Q, then s sign bits, then the strict upper part row-major."""
    P, Q = list(range(s)), list(range(s))
    for perm in (P, Q):
        for i in range(s, 1, -1):
            j = rng.next() % i
            perm[i - 1], perm[j] = perm[j], perm[i - 1]
    D = [rng.next() & 1 for _ in range(s)]
    M = [[0] * s for _ in range(s)]
    for i in range(s):
        M[P[i]][Q[i]] = 1 if D[i] else -1
        for j in range(i + 1, s):
            M[P[i]][Q[j]] = rng.next() % 3 - 1
    return M


def identity(s):
    return [[1 if i == j else 0 for j in range(s)] for i in range(s)]


def candidate_uvw(m, k, n, seed):
    if seed == BASE_SEED:
        return identity(m), identity(k), identity(n)
    rng = CandRng(seed)
    U = zoi_matrix(rng, m)
    V = zoi_matrix(rng, k)
    W = zoi_matrix(rng, n)
    return U, V, W


def inverse(M):
    """Gauss-Jordan over Q with row pivoting."""
    s = len(M)
    A = [[Fraction(x) for x in row] + [Fraction(int(i == j)) for j in range(s)] for i, row in enumerate(M)]
    for c in range(s):
        r = next(i for i in range(c, s) if A[i][c] != 0)
        A[c], A[r] = A[r], A[c]
        pv = A[c][c]
        A[c] = [x / pv for x in A[c]]
        for i in range(s):
            if i != c and A[i][c] != 0:
                f = A[i][c]
                A[i] = [a - f * b for a, b in zip(A[i], A[c])]
    return [row[s:] for row in A]


def transpose(M):
    return [list(r) for r in zip(*M)]


def tensor(A, B):
    ra, ca, rb, cb = len(A), len(A[0]), len(B), len(B[0])
    T = [[Fraction(0)] * (ca * cb) for _ in range(ra * rb)]
    for i in range(ra):
        for j in range(ca):
            if A[i][j] != 0:
                for u in range(rb):
                    for v in range(cb):
                        T[i * rb + u][j * cb + v] = Fraction(A[i][j]) * B[u][v]
    return T


def dense(m, n, ent):
    M = [[Fraction(0)] * n for _ in range(m)]
    for (i, j), v in ent.items():
        M[i][j] = Fraction(v)
    return M


def small_ints(A):
    """A as an int64 array when every entry is an integer below 2^20 in size, else None"""
    if isinstance(A, np.ndarray):
        return A
    if all(x.denominator == 1 and abs(x.numerator) < (1 << 20) for row in A for x in row):
        return np.array([[int(x) for x in row] for row in A], dtype=np.int64)
    return None


def matmul(A, B):
    """Exact dense product: int64 numpy when both sides hold small integers (|sums| < 2^(40 + log2 of the inner
    dimension) < 2^63), Fractions otherwise."""
    a, b = small_ints(A), small_ints(B)
    if a is not None and b is not None and b.shape[0] < (1 << 20):
        return a @ b
    A = A.tolist() if isinstance(A, np.ndarray) else A
    B = B.tolist() if isinstance(B, np.ndarray) else B
    A = [[Fraction(x) for x in row] for row in A]
    B = [[Fraction(x) for x in row] for row in B]
    n, kk = len(B[0]), len(B)
    return [[sum((A[i][t] * B[t][j] for t in range(kk) if A[i][t] != 0 and B[t][j] != 0), Fraction(0)) for j in range(n)] for i in range(len(A))]


def shape(L, R, P):
    """(m, k, n) of a triple given as (rows, cols) pairs, or None: L is r x mk, R is r x kn, P is mn x r."""
    (lr, lc), (rr, rc), (pr, pc) = L, R, P
    if lr != rr or lr != pc or lc == 0:
        return None
    if (rc * pr) % lc:
        return None
    q = rc * pr // lc
    n = int(round(q ** 0.5))
    while n * n > q:
        n -= 1
    while (n + 1) * (n + 1) <= q:
        n += 1
    if n == 0 or n * n != q or pr % n or rc % n:
        return None
    m, k = pr // n, rc // n
    if m * k != lc or k * n != rc or m * n != pr:
        return None
    return m, k, n


def load(base):
    """The triple base_{L,R,P}.sms as dense Fraction matrices and its shape."""
    mats = [read_sms(base + "_%s.sms" % x) for x in "LRP"]
    sh = shape(*[(a, b) for a, b, _ in mats])
    mats = [dense(*t) for t in mats]
    return [M if small_ints(M) is None else small_ints(M) for M in mats], sh


def reduce_mod(x, p):
    x = Fraction(x)
    return (x.numerator % p) * pow(x.denominator % p, -1, p) % p


def products(mats, mkn, seed):
    L, R, P = mats
    m, k, n = mkn
    U, V, W = candidate_uvw(m, k, n, seed)
    J = tensor(inverse(U), V)
    G = tensor(transpose(inverse(V)), W)
    H = tensor(U, inverse(W))
    return matmul(L, J), matmul(R, G), matmul(H, P)


def counts(Lj, Rg, hP, modulus=0, measure=DENSITY):
    """(cost, nnz, nno) of the three products"""
    Lj, Rg, hP = [M.tolist() if isinstance(M, np.ndarray) else M for M in (Lj, Rg, hP)]
    if modulus:
        red = lambda M: [[reduce_mod(x, modulus) for x in row] for row in M]  # noqa: E731
        Lj, Rg, hP = red(Lj), red(Rg), red(hP)
        one = lambda x: x == 1 or x == modulus - 1  # noqa: E731
    else:
        one = lambda x: x == 1 or x == -1  # noqa: E731
    nnz = nno = canon = 0
    for M, rows in ((Lj, Lj), (Rg, Rg), (hP, transpose(hP))):
        for row in rows:
            c = sum(1 for x in row if x != 0)
            nnz += c
            nno += sum(1 for x in row if x != 0 and not one(x))
            canon += c == 1
    if measure == CANONICAL and not modulus:
        cost = len(Lj) + len(Rg) + len(hP[0]) - canon
    else:
        cost = nnz
    return cost, nnz, nno


def cost3(mats, mkn, seed, modulus=0, measure=DENSITY):
    return counts(*products(mats, mkn, seed), modulus=modulus, measure=measure)


def mm_check(Lj, Rg, hP, mkn, modulus=0):
    """Exact Brent equations of a row-major triple: sum_r L[r][a k + b] R[r][b' n + c] P[a' n + c'][r] equals
    [a == a'][b == b'][c == c'] over Q, or modulo `modulus`."""
    m, k, n = mkn
    r = len(Lj)
    ok = lambda x: (x % modulus if modulus else x) == 0  # noqa: E731
    conv = (lambda x: reduce_mod(x, modulus)) if modulus else (lambda x: x)
    Lj, Rg, hP = [M.tolist() if isinstance(M, np.ndarray) else M for M in (Lj, Rg, hP)]
    Lm = [[conv(x) for x in row] for row in Lj]
    Rm = [[conv(x) for x in row] for row in Rg]
    Pm = [[conv(x) for x in row] for row in hP]
    for a in range(m):
        for b in range(k):
            for b2 in range(k):
                for c in range(n):
                    lr = [(t, Lm[t][a * k + b] * Rm[t][b2 * n + c]) for t in range(r) if Lm[t][a * k + b] != 0 and Rm[t][b2 * n + c] != 0]
                    for a2 in range(m):
                        for c2 in range(n):
                            s = sum((v * Pm[a2 * n + c2][t] for t, v in lr), 0)
                            want = 1 if (a == a2 and b == b2 and c == c2) else 0
                            if not ok(s - want):
                                return False
    return True
