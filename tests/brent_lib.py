"""Helpers of the Brent-equation tests (bin/MMchecker, plo_brent_*): an oracle that shares no code with the product, and the
triples the tests feed it.

A matrix is (rows, columns, {(i, j): Fraction}) as plo_testlib.read_sms returns it; a triple is (L, R, P, (m, k, n)) with L r x mk,
R r x kn, P mn x r.  With x = a k + b, y = b' n + c, z = a' n + c', equation e = (x kn + y) mn + z asks
    S[x][y][z] = sum_t L[t][x] R[t][y] P[z][t] == [a = a'][b = b'][c = c'].
The oracle builds S one t at a time (an outer product of the three rows) modulo q in int64, or over Q in Fractions, and
returns (violated, first, value): the number of violated equations, the smallest e (None when there is none) and S there."""
import functools
import os
import random
from fractions import Fraction

import numpy as np

import orbit_oracle
from plo_testlib import DATA, read_sms

P31 = 2147483629


def load(name):
    mats = [read_sms(os.path.join(DATA, "%s_%s.sms" % (name, x))) for x in "LRP"]
    sh = orbit_oracle.shape(*[(a, b) for a, b, _ in mats])
    assert sh is not None, name
    return mats[0], mats[1], mats[2], sh


def naive(m, k, n):
    """r = mkn products a[a][b] b[b][c], one per (a, b, c)"""
    L, R, P = {}, {}, {}
    for a in range(m):
        for b in range(k):
            for c in range(n):
                t = (a * k + b) * n + c
                L[(t, a * k + b)] = Fraction(1); R[(t, b * n + c)] = Fraction(1); P[(a * n + c, t)] = Fraction(1)
    r = m * k * n
    return (r, m * k, L), (r, k * n, R), (m * n, r, P), (m, k, n)


def tensor(A, B):
    """The tensor product of two triples: (m1 m2) x (k1 k2) x (n1 n2) of rank r1 r2, the columns permuted to row-major order"""
    (_, _, LA), (_, _, RA), (_, _, PA), (m1, k1, n1) = A
    (rb, _, LB), (_, _, RB), (_, _, PB), (m2, k2, n2) = B
    ra = A[0][0]
    m, k, n = m1 * m2, k1 * k2, n1 * n2

    def idx(i1, i2, rows1, cols1, rows2, cols2):                       # entry (u1, v1) of block 1 and (u2, v2) of block 2
        u1, v1 = divmod(i1, cols1); u2, v2 = divmod(i2, cols2)
        return (u1 * rows2 + u2) * (cols1 * cols2) + v1 * cols2 + v2

    L, R, P = {}, {}, {}
    for (t1, x1), v1 in LA.items():
        for (t2, x2), v2 in LB.items():
            L[(t1 * rb + t2, idx(x1, x2, m1, k1, m2, k2))] = v1 * v2
    for (t1, y1), v1 in RA.items():
        for (t2, y2), v2 in RB.items():
            R[(t1 * rb + t2, idx(y1, y2, k1, n1, k2, n2))] = v1 * v2
    for (z1, t1), v1 in PA.items():
        for (z2, t2), v2 in PB.items():
            P[(idx(z1, z2, m1, n1, m2, n2), t1 * rb + t2)] = v1 * v2
    r = ra * rb
    return (r, m * k, L), (r, k * n, R), (m * n, r, P), (m, k, n)


def residue(v, q):
    v = Fraction(v)
    return v.numerator % q * pow(v.denominator % q, -1, q) % q


def dense_mod(M, q):
    rows, cols, ent = M
    A = np.zeros((rows, cols), dtype=np.int64)
    for (i, j), v in ent.items():
        A[i, j] = residue(v, q)
    return A


def from_dense(A):
    A = np.asarray(A)
    return A.shape[0], A.shape[1], {(int(i), int(j)): Fraction(int(A[i, j])) for i, j in zip(*np.nonzero(A))}


def matmul_mod(A, B, q):
    """(A B) mod q for residues below 2^31: B in two 16-bit halves, so that every int64 sum stays below 2^63"""
    A = np.asarray(A, dtype=np.int64); B = np.asarray(B, dtype=np.int64)
    assert A.shape[1] < (1 << 15)
    hi, lo = B >> 16, B & 0xFFFF
    return ((A @ hi % q) * 65536 + A @ lo) % q


def inverse_mod(M, q):
    """the inverse of a square matrix modulo a prime, or None"""
    s = len(M)
    A = [[int(x) % q for x in row] + [int(i == j) for j in range(s)] for i, row in enumerate(M)]
    for c in range(s):
        piv = next((i for i in range(c, s) if A[i][c]), None)
        if piv is None:
            return None
        A[c], A[piv] = A[piv], A[c]
        inv = pow(A[c][c], -1, q)
        A[c] = [x * inv % q for x in A[c]]
        for i in range(s):
            if i != c and A[i][c]:
                f = A[i][c]
                A[i] = [(x - f * y) % q for x, y in zip(A[i], A[c])]
    return [row[s:] for row in A]


def change_basis(T, q, seed):
    """L (U^-1 (x) V), R (V^-T (x) W), (U (x) W^-1) P modulo the prime q for random invertible U, V, W: every row becomes dense
    and the triple stays a multiplication algorithm"""
    L, R, P, (m, k, n) = T
    rng = random.Random(seed)

    def draw(s):
        while True:
            M = [[rng.randrange(q) for _ in range(s)] for _ in range(s)]
            Mi = inverse_mod(M, q)
            if Mi is not None:
                return np.array(M, dtype=np.int64), np.array(Mi, dtype=np.int64)

    (U, Ui), (V, Vi), (W, Wi) = draw(m), draw(k), draw(n)
    kron = lambda A, B: np.kron(A, B) % q  # noqa: E731   (products below 2^62)
    L2 = matmul_mod(dense_mod(L, q), kron(Ui, V), q)
    R2 = matmul_mod(dense_mod(R, q), kron(Vi.T, W), q)
    P2 = matmul_mod(kron(U, Wi), dense_mod(P, q), q)
    return from_dense(L2), from_dense(R2), from_dense(P2), (m, k, n)


def changed(T, which, i, j, value):
    """the triple with one entry of L (0), R (1) or P (2) set to `value` (0 removes it)"""
    mats = [(a, b, dict(ent)) for a, b, ent in T[:3]]
    if value == 0:
        mats[which][2].pop((i, j), None)
    else:
        mats[which][2][(i, j)] = Fraction(value)
    return mats[0], mats[1], mats[2], T[3]


def expected(mkn):
    m, k, n = mkn
    E = np.zeros((m * k, k * n, m * n), dtype=np.int64)
    for a in range(m):
        for b in range(k):
            for c in range(n):
                E[a * k + b, b * n + c, a * n + c] = 1
    return E


def _verdict(S, E):
    bad = S != E
    cnt = int(np.count_nonzero(bad))
    if cnt == 0:
        return 0, None, None
    e = int(np.argmax(bad.reshape(-1)))
    return cnt, e, S.reshape(-1)[e]


def sums_mod(T, q):
    """S modulo q as an (mk, kn, mn) int64 array"""
    L, R, P, (m, k, n) = T
    Lq, Rq, PTq = dense_mod(L, q), dense_mod(R, q), dense_mod(P, q).T.copy()
    S = np.zeros((m * k, k * n, m * n), dtype=np.int64)
    for t in range(L[0]):
        xs, ys, zs = np.nonzero(Lq[t])[0], np.nonzero(Rq[t])[0], np.nonzero(PTq[t])[0]
        if len(xs) == 0 or len(ys) == 0 or len(zs) == 0:
            continue
        lr = Lq[t, xs][:, None] * Rq[t, ys][None, :] % q                          # below 2^62, then below q
        term = lr[:, :, None] * PTq[t, zs][None, None, :]
        term %= q
        if term.shape == S.shape:
            S += term                                                             # r < 2^32 terms below 2^31: no overflow before the end
        else:
            S[np.ix_(xs, ys, zs)] += term
    S %= q
    return S


def oracle_mod(T, q, pair0=0, pair1=None):
    """(violated, first, value) among the pairs [pair0, pair1) modulo q"""
    S, E = sums_mod(T, q), expected(T[3])
    mn = S.shape[2]
    S, E = S.reshape(-1, mn), E.reshape(-1, mn)
    pair1 = S.shape[0] if pair1 is None else pair1
    cnt, e, v = _verdict(S[pair0:pair1], E[pair0:pair1] % q)
    return (cnt, None, None) if cnt == 0 else (cnt, e + pair0 * mn, int(v))


def oracle_q(T):
    """(violated, first, value) over Q, in Fractions"""
    L, R, P, (m, k, n) = T
    S = np.full((m * k, k * n, m * n), Fraction(0), dtype=object)
    rows = lambda M, tr: {t: [(j if not tr else i, v) for (i, j), v in M[2].items() if (i if not tr else j) == t] for t in range(L[0])}  # noqa: E731
    Lr, Rr, Pr = rows(L, False), rows(R, False), rows(P, True)
    for t in range(L[0]):
        if not (Lr[t] and Rr[t] and Pr[t]):
            continue
        lv = np.array([v for _, v in Lr[t]], dtype=object); rv = np.array([v for _, v in Rr[t]], dtype=object); pv = np.array([v for _, v in Pr[t]], dtype=object)
        ix = np.ix_([x for x, _ in Lr[t]], [y for y, _ in Rr[t]], [z for z, _ in Pr[t]])
        S[ix] = S[ix] + np.einsum("x,y,z->xyz", lv, rv, pv)
    cnt, e, v = _verdict(S, expected(T[3]).astype(object))
    return (cnt, None, None) if cnt == 0 else (cnt, e, Fraction(v))


def sum_at(T, e):
    """S over Q at equation e alone: one sum of Fractions over t"""
    L, R, P, (m, k, n) = T
    pair, z = divmod(e, m * n)
    x, y = divmod(pair, k * n)
    zero = Fraction(0)
    return sum((L[2].get((t, x), zero) * R[2].get((t, y), zero) * P[2].get((z, t), zero) for t in range(L[0])), zero)


def bits(v):
    return abs(int(v)).bit_length()


def certificate(T):
    """(beta, j) of the proof over Q: beta = bits(r) + sum over the matrices of the longest numerator and of the bits of the
    distinct denominators above 1, + 2; j = ceil(beta / 30)"""
    beta = bits(T[0][0]) + 2
    for M in T[:3]:
        beta += max([bits(v.numerator) for v in M[2].values()] or [0])
        beta += sum(bits(d) for d in {v.denominator for v in M[2].values()} if d > 1)
    return beta, -(-beta // 30)


def csr(M):
    """(rows, columns, rowptr, col, num, den) for plinopt_amd.BrentPlan"""
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


def write_sms(path, M):
    rows, cols, ent = M
    with open(path, "w") as f:
        f.write("%d %d R\n" % (rows, cols))
        for (i, j), v in sorted(ent.items()):
            f.write("%d %d %s\n" % (i + 1, j + 1, v))
        f.write("0 0 0\n")


def write_triple(tmp, T, stem="t"):
    names = [os.path.join(str(tmp), "%s_%s.sms" % (stem, x)) for x in "LRP"]
    for p, M in zip(names, T[:3]):
        write_sms(p, M)
    return names


def indices(e, mkn):
    """(a, b, b', c, a', c') of equation e"""
    m, k, n = mkn
    pair, z = divmod(e, m * n)
    x, y = divmod(pair, k * n)
    return x // k, x % k, y // n, y % n, z // n, z % n


@functools.lru_cache(maxsize=None)
def tensor_6x6x12():
    return tensor(load("3x3x6_40"), load("2x2x2_7_Winograd"))


@functools.lru_cache(maxsize=None)
def tensor_6x6x12_dense():
    return change_basis(tensor_6x6x12(), P31, 7)
