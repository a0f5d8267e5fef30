"""Batches for plo_cse_batch_search (tests/test_gpu_cse_batch.py): problems as (m, n, rowptr, col, val) with their oracle
matrices, and the expected minima from the C oracle -- OracleMatrix.search over the seeds of a problem, or the argmin of
oracle_chain over them for a chained problem.  Nothing here runs the code under test."""
import os
from types import SimpleNamespace

import synth
from plo_testlib import DATA, OracleMatrix, oracle_chain, read_sms, to_csr_mod
from test_gpu_chain_synth import tight_general, tight_unit  # noqa: F401  (re-exported for the tests)

P = synth.CHAIN_PRIME
_search, _chain = {}, {}


def from_rows(name, m, n, rows, p=P):
    rows = [{j: v % p for j, v in r.items() if v % p} for r in rows]
    csr = (m, n) + synth.to_csr(rows, p)
    return SimpleNamespace(name=name, m=m, n=n, rows=rows, p=p, csr=csr, O=OracleMatrix(*(csr + (p,))), plan=synth.wave_plan(m, n, rows, p))


def from_sms(fname, p=P):
    m, n, ent = read_sms(os.path.join(DATA, fname))
    rp, c, v = to_csr_mod(m, n, ent, p)
    rows = [{c[k]: v[k] for k in range(rp[i], rp[i + 1])} for i in range(m)]
    return from_rows(fname, m, n, rows, p)


def key(ops, seed, mode=0):
    a, mu = ops
    return ((a + mu, a), (a, mu), (a + mu,))[mode] + (seed,)


def expected(prob, seed0, per, mode=0):
    """(adds, muls, seed) of the oracle's minimum under (cost key of mode, seed) over seed0 .. seed0+per-1"""
    k = (prob.name, prob.p, seed0, per, mode)
    if k not in _search:
        if mode == 2:                                   # the oracle's sum-only search does not return the split: argmin over its costs
            a, mu = prob.O.cost_many(seed0=seed0, nseeds=per, nthreads=4)
            j = min(range(per), key=lambda j: key((a[j], mu[j]), seed0 + j, 2))
            _search[k] = (a[j], mu[j], seed0 + j)
        else:
            _search[k] = prob.O.search(seed0, per, mode, nthreads=4)
    return _search[k]


def expected_chain(A, B, seed0, per, mode=0):
    out = []
    for s in range(seed0, seed0 + per):
        k = (A.name, B.name, A.p, s)
        if k not in _chain:
            _chain[k] = oracle_chain(A.O, B.O, s)
        out.append(_chain[k])
    j = min(range(per), key=lambda j: key(out[j], seed0 + j, mode))
    return out[j] + (seed0 + j,)


def mixed40():
    """40 problems of different sizes, unit and general alternating while both last: data matrices, small_valued and sweep
    matrices, a matrix whose rows all have one entry (no pair at all), one with an empty row, one without entries"""
    data = [from_sms(f) for f in ("2x2x2_7_Winograd_L.sms", "cyclic.sms", "4x4x4_49_156_L.sms", "4x4x4_49_156_P.sms", "4x4x4_48_rational_P.sms", "2x2x2_7_DPS-accurate_L.sms")]
    edge = [from_rows("one_entry_rows", 5, 4, [{0: 1}, {1: 3}, {3: -1}, {0: 2}, {2: 1}]),
            from_rows("empty_row", 4, 3, [{0: 1, 1: 1, 2: 1}, {}, {0: 1, 1: 1}, {1: 2, 2: 2}]),
            from_rows("no_entries", 3, 2, [{}, {}, {}])]
    small = [from_rows("small_valued_%d" % s, *synth.small_valued(s, P)) for s in range(17)]
    sweeps = [from_rows("sweep_%d" % s, *synth.sweep(100 + s, P, 9 + 3 * s, 8 + 2 * s)) for s in range(7)]
    units = [from_rows("unit_%d" % s, *synth.sweep(200 + s, P, 6 + 5 * s, 5 + 3 * s, density=0.5, unit_frac=1.0)) for s in range(7)]
    every = data + edge + small + sweeps + units
    assert len(every) == 40 and all(not isinstance(x.plan, str) for x in every)
    u, g = [x for x in every if x.plan.unit], [x for x in every if not x.plan.unit]
    out = []
    while u or g:
        if u:
            out.append(u.pop(0))
        if g:
            out.append(g.pop(0))
    assert sum(1 for a, b in zip(out, out[1:]) if a.plan.unit != b.plan.unit) >= 20
    sizes = sorted(x.plan.region_bytes for x in out)
    assert sizes[-1] > 16 * sizes[0]                     # large and small footprints in one batch
    return out


def chained12():
    """12 pairs of chain_cases(): the families built to tell a continued random stream from a restarted one"""
    every = [c for c in synth.chain_cases() if c.p == P and not c.refusal]
    cs = [c for fam in ("order", "silent", "dispatch") for c in [c for c in every if c.family == fam][:4]]
    assert len(cs) == 12
    conv = lambda c, x, tag: SimpleNamespace(name=c.name + tag, m=x.m, n=x.n, rows=x.rows, p=c.p, csr=x.csr, O=OracleMatrix(*(x.csr + (c.p,))))   # noqa: E731
    return [(conv(c, c.A, ":A"), conv(c, c.B, ":B")) for c in cs]


def refused():
    """a matrix synth.wave_plan says the wave kernel refuses (65 rows, one coefficient other than +-1), and the code's name"""
    c = next(c for c in synth.chain_cases() if c.name == "chain_refuse_gen65x2_first")
    assert synth.wave_plan(c.A.m, c.A.n, c.A.rows, c.p) == "PLO_E_CAPACITY"
    return SimpleNamespace(name="gen65x2", csr=c.A.csr, p=c.p), "PLO_E_CAPACITY"
