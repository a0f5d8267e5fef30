"""Literal oracle of the two other candidate distributions of the De Groote orbit search (bin/orbiter --action pluq and
--action householder; reference src/orbiter.cpp:77-96 ACTION_FULL_PLUQ and :98-123 ACTION_HOUSEHOLDER), restated from the
stream text of include/plinopt_hip.h (PLO_ORBIT_ACT_*) as dense matrices over fractions.Fraction.  The matrices go the way of
tests/orbit_oracle.py: Gauss-Jordan inverses, literal Kronecker products, dense products, `counts`, `mm_check`.  Nothing here
knows that a PLUQ matrix is a product of triangles or that a Householder matrix is its own inverse up to signs.

Every action starts alike: P by Fisher-Yates, then Q, then D[i] = next() & 1.
  PLUQ         Lambda lower triangular, Lambda[i][i] = D[i] ? 1 : -1, then row-major for j < i one draw next() % 3 - 1 each;
               then for i = 0..s-1 a vector u with u[Q[i]] = 1, u[j] = next() % 3 - 1 for j = 0..Q[i]-1 and zeros behind;
               row P[i] of M is Lambda.u.
  HOUSEHOLDER  u[i] = next() % 3 - 1, d = sum u[i]^2; when d is a unit of the run's field (d != 0 over Q, gcd(d, modulus) = 1
               modulo a number) M[P[i]][Q[j]] = +-(delta_ij - 2 u[i] u[j] / d) with the sign of D[i], else the signed
               permutation M[P[i]][Q[i]] = +-1."""
from fractions import Fraction
from math import gcd

import orbit_oracle as O

TRIANGULAR, PLUQ, HOUSEHOLDER = 0, 1, 2
ACTIONS = {"triangular": TRIANGULAR, "pluq": PLUQ, "householder": HOUSEHOLDER}
BASE_SEED = O.BASE_SEED


def is_unit(d, modulus):
    return d != 0 if not modulus else gcd(d, modulus) == 1


def _start(rng, s):
    P, Q = list(range(s)), list(range(s))
    for perm in (P, Q):
        for i in range(s, 1, -1):
            j = rng.next() % i
            perm[i - 1], perm[j] = perm[j], perm[i - 1]
    D = [rng.next() & 1 for _ in range(s)]
    return P, Q, D


def pluq_matrix(rng, s):
    P, Q, D = _start(rng, s)
    lam = [[0] * s for _ in range(s)]
    for i in range(s):
        lam[i][i] = 1 if D[i] else -1
    for i in range(s):
        for j in range(i):
            lam[i][j] = rng.next() % 3 - 1
    M = [[0] * s for _ in range(s)]
    for i in range(s):
        u = [0] * s
        u[Q[i]] = 1
        for j in range(Q[i]):
            u[j] = rng.next() % 3 - 1
        M[P[i]] = [sum(lam[c][j] * u[j] for j in range(s)) for c in range(s)]
    return M


def householder_matrix(rng, s, modulus=0, trace=None):
    """trace, when given, collects (s, d) of every matrix drawn"""
    P, Q, D = _start(rng, s)
    u = [rng.next() % 3 - 1 for _ in range(s)]
    d = sum(x * x for x in u)
    if trace is not None:
        trace.append((s, d))
    M = [[Fraction(0)] * s for _ in range(s)]
    for i in range(s):
        sign = 1 if D[i] else -1
        if is_unit(d, modulus):
            for j in range(s):
                M[P[i]][Q[j]] = sign * (Fraction(int(i == j)) - Fraction(2 * u[i] * u[j], d))
        else:
            M[P[i]][Q[i]] = Fraction(sign)
    return M


def candidate_uvw(m, k, n, seed, action, modulus=0, trace=None):
    if seed == BASE_SEED:
        return O.identity(m), O.identity(k), O.identity(n)
    rng = O.CandRng(seed)
    if action == TRIANGULAR:
        return [O.zoi_matrix(rng, s) for s in (m, k, n)]
    if action == PLUQ:
        return [pluq_matrix(rng, s) for s in (m, k, n)]
    assert action == HOUSEHOLDER
    return [householder_matrix(rng, s, modulus, trace) for s in (m, k, n)]


def householder_ds(mkn, seed, modulus=0):
    """[(size, d)] of U, V and W of the seed's Householder candidate"""
    trace = []
    candidate_uvw(*mkn, seed, HOUSEHOLDER, modulus, trace)
    return trace


def products(mats, mkn, seed, action, modulus=0):
    L, R, P = mats
    U, V, W = candidate_uvw(*mkn, seed, action, modulus)
    J = O.tensor(O.inverse(U), V)
    G = O.tensor(O.transpose(O.inverse(V)), W)
    H = O.tensor(U, O.inverse(W))
    return O.matmul(L, J), O.matmul(R, G), O.matmul(H, P)


def cost3(mats, mkn, seed, action, modulus=0, measure=O.DENSITY):
    return O.counts(*products(mats, mkn, seed, action, modulus), modulus=modulus, measure=measure)
