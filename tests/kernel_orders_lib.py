"""Shared by test_gpu_kernel_orders.py and test_kernel_orders_host.py: the walk of `bin/optimizer -N` by order index
(`plo_kernel_search_orders`) restated from the oracle's prescribed-order decomposition (`OracleMatrix.kernel_order`).

Candidate c of a range [first, first + count) with `sub` restarts per order is restart j = c % sub of order index
pi = first + c // sub: the pi-th permutation of the rows in lexicographic order, the decomposition's stream seeded
seed0 + pi, the two Optimizer calls seeded seed0 + pi * sub + j."""
import functools
import math
import os

import numpy as np

from plo_testlib import DATA, OracleMatrix

P = 131071


def kth_permutation(m, k):
    """the k-th permutation of 0..m-1 in lexicographic order (digits of k in the factorial base)"""
    left, out = list(range(m)), []
    for i in range(m):
        d, k = divmod(k, math.factorial(m - 1 - i))
        out.append(left.pop(d))
    return out


def cost_key(adds, muls, cost_mode):
    return {0: (adds + muls, adds), 1: (adds, muls), 2: (adds + muls,)}[cost_mode]


@functools.lru_cache(maxsize=None)
def fixture(name):
    return OracleMatrix.from_sms(os.path.join(DATA, name + ".sms"), P)


def matrix_from_rows(rows, n):
    rp, c, v = [0], [], []
    for r in rows:
        for j, x in enumerate(r):
            if x % P:
                c.append(j); v.append(int(x) % P)
        rp.append(len(c))
    return OracleMatrix(len(rows), n, rp, c, v, P)


@functools.lru_cache(maxsize=None)
def synthetic12(kind):
    """The two 12 x 6 matrices of the 12-row cases, from fixed numpy seeds.  "mixed": entries in {0, +-1, 2, 3}, row 4 empty, row 9
    equal to row 2.  "unit": entries +-1 and 0 only (the kernel's +-1 instantiation).  The seeds are the first ones tried (2026 and
    2027); both matrices meet the 30-distinct-results condition of the tests on every range used."""
    if kind == "mixed":
        rng = np.random.RandomState(2026)
        A = rng.choice([0, 0, 0, 1, -1, 2, 3], size=(12, 6))
        A[4, :] = 0
        A[9, :] = A[2, :]
    else:
        rng = np.random.RandomState(2027)
        A = rng.choice([0, 0, 1, -1], size=(12, 6))
    return matrix_from_rows(A.tolist(), 6)


@functools.lru_cache(maxsize=None)
def oracle_range(M, seed0, first, count, sub):
    """[(adds, muls, rank, NotIndep, kept dependent rows)] of the count * sub candidates, computed once per session"""
    out = []
    for pi in range(first, first + count):
        order = kth_permutation(M.m, pi)
        for j in range(sub):
            a, mu, rank, ni, sig = M.kernel_order(order, seed0 + pi, seed0 + pi * sub + j)
            kept = next(i for i, x in enumerate(sig) if x >= M.m)          # the signature lists the kept dependent rows, then m + NotIndep
            out.append((a, mu, rank, ni, kept))
    return tuple(out)


def oracle_best(exp, seed0, first, sub, cost_mode=0):
    """(adds, muls, seed) of the first minimum under (key, candidate index), as plo_best_t reports it (the sum alone in .adds for PLO_COST_SUM)"""
    k = min(range(len(exp)), key=lambda k: (cost_key(exp[k][0], exp[k][1], cost_mode), k))
    a, mu = exp[k][:2]
    return (a + mu, 0, seed0 + first * sub + k) if cost_mode == 2 else (a, mu, seed0 + first * sub + k)


def distinct(exp):
    return len({(a, mu, r, ni) for a, mu, r, ni, _ in exp})


def csr_args(M):
    return (M.m, M.n, M.rowptr, M.col, M.val)
