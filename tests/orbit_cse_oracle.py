"""Literal oracle of the CSE measure of the De Groote orbit search (bin/orbiter -z, PLO_ORBIT_CSE of include/plinopt_hip.h;
reference src/orbiter.cpp:172-209).  A composition of what the suite already trusts and no product code: the dense products
of tests/orbit_oracle.py (or tests/orbit_action_oracle.py for the other actions) reduced modulo p with the zeros dropped, each
part handed to the CPU oracle as a plo_testlib.OracleMatrix, and

    c(M) = min(sum(naive_ops(M)), min over the seeds cse_seed0 .. cse_seed0 + sub - 1 of adds + muls of cost_many),
    cost = c(Lj) + c(Rg) + c(hP);  a matrix without entries costs 0.

nnz and nno are those of orbit_oracle.counts."""
import numpy as np

import orbit_action_oracle as A
import orbit_oracle as O
from plo_testlib import OracleMatrix

BASE_SEED = O.BASE_SEED
CSE = 1


def reduced(M, p):
    """CSR (m, n, rowptr, col, val) of the dense product M modulo p, zeros dropped"""
    M = M.tolist() if isinstance(M, np.ndarray) else M
    rp, col, val = [0], [], []
    for row in M:
        for j, x in enumerate(row):
            v = O.reduce_mod(x, p)
            if v:
                col.append(j)
                val.append(v)
        rp.append(len(col))
    return len(M), len(M[0]) if M else 0, rp, col, val


def part_cost(M, p, sub, cse_seed0):
    m, n, rp, col, val = reduced(M, p)
    if not val:
        return 0
    om = OracleMatrix(m, n, rp, col, val, p)
    adds, muls = om.cost_many(seed0=cse_seed0, nseeds=sub)
    return min(sum(om.naive_ops()), min(a + b for a, b in zip(adds, muls)))


def cost3(mats, mkn, seed, p, sub=1, cse_seed0=0, action=A.TRIANGULAR):
    """(cost, nnz, nno) of candidate `seed`"""
    prods = O.products(mats, mkn, seed) if action == A.TRIANGULAR else A.products(mats, mkn, seed, action, p)
    _, nnz, nno = O.counts(*prods, modulus=p)
    return sum(part_cost(M, p, sub, cse_seed0) for M in prods), nnz, nno


def costs(mats, mkn, seeds, p, sub=1, cse_seed0=0, action=A.TRIANGULAR):
    """[(cost, nnz, nno)] per seed and the lexicographic argmin (cost, nnz, nno, seed); the base seed orders as itself (2^64 - 1)"""
    out = [cost3(mats, mkn, s, p, sub, cse_seed0, action) for s in seeds]
    return out, min(c + (s,) for c, s in zip(out, seeds))
