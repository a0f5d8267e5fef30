"""The matrices of the exact CSE restart search over Q (plo_cse_plan_create_q, bin/optimizer --gpu-q) and what each must do:
run (then tests/golden/cse_q_costs.json holds its per-seed costs from tests/cse_q_oracle.py) or be refused with a code.

- the rational fixtures;
- the shapes of the edge cases of the one-wave kernel (synth.cse_cases(), imported read-only), their residues mapped onto
  {+-1, +-2, +-1/2, 3, -1/3}: +-1 stay, the other residues of a case take the six values in turn.  The `moduli` family repeats two
  shapes under seven moduli: only the 31-bit instances are kept;
- tie_order: a column pair tied at two ratios whose order over Q and whose order as residues disagree; its costs differ from the
  costs modulo 2147483629 on 10 of the seeds 0..31 (tests/test_cse_q_host.py checks it with the two oracles);
- triangle: Triangle fires;
- values64 / values65: exactly 64 distinct values (runs), 65 (refused);
- prime_step: a numerator that 2147483629 divides: the next prime below is taken;
- collide: the entries 1 and 2^30 + 4 meet on one residue modulo the prime 2^30 + 3: with PLO_CSE_Q_PRIME set to it (colliding_prime
  finds it from U alone) the plan takes the next prime below;
- overflow: entries of 61-bit numerators and denominators: their ratios cannot be ordered in 128 bits (refused).
"""
import os
from fractions import Fraction as F
from types import SimpleNamespace

import synth
from plo_testlib import DATA, read_sms

PRIME0 = 2147483629
FIXTURES = ["2x2x2_7_Winograd_L", "2x2x2_7_DPS-accurate_L", "4x4x4_48_rational_L", "4x4x4_48_rational_P", "3x4x7_63_rational_R", "4o4o8_Toom5_P"]
FIXTURE_SEEDS = {"4x4x4_48_rational_L": 150}                     # the others: 64
TINY_SEEDS = 256
MAPPED = [F(2), F(-2), F(1, 2), F(-1, 2), F(3), F(-1, 3)]
UNSUPPORTED = -4                                                 # PLO_E_UNSUPPORTED


def _case(out, name, m, n, ent, nseeds=TINY_SEEDS, refused=None, why=None, fixture=None):
    assert name not in [c.name for c in out], name
    out.append(SimpleNamespace(name=name, m=m, n=n, ent=dict(ent), nseeds=0 if refused else nseeds, refused=refused, why=why, fixture=fixture))
    return out[-1]


def _rows_ent(rows):
    return {(i, j): F(v) for i, r in enumerate(rows) for j, v in r.items()}


def mapped_entries(c):
    """the entries of a synthetic case of the wave kernel over Q: residues 1 and p - 1 are +-1, the others take MAPPED in turn"""
    others = sorted({v for r in c.rows for v in r.values()} - {1, c.p - 1})
    to = {1: F(1), c.p - 1: F(-1)}
    to.update({v: MAPPED[k % len(MAPPED)] for k, v in enumerate(others)})
    return {(i, j): to[v] for i, r in enumerate(c.rows) for j, v in r.items()}


def csr_q(c):
    """(m, n, rowptr, col, num, den) of a case"""
    rows = [[] for _ in range(c.m)]
    for (i, j), v in sorted(c.ent.items()):
        rows[i].append((j, v))
    rp, col, num, den = [0], [], [], []
    for r in rows:
        for j, v in r:
            col.append(j)
            num.append(v.numerator)
            den.append(v.denominator)
        rp.append(len(col))
    return c.m, c.n, rp, col, num, den


def sms_text(c):
    lines = ["%d %d R" % (c.m, c.n)] + ["%d %d %s" % (i + 1, j + 1, v) for (i, j), v in sorted(c.ent.items())] + ["0 0 0"]
    return "\n".join(lines) + "\n"


def cases():
    out = []
    for name in FIXTURES:
        m, n, ent = read_sms(os.path.join(DATA, name + ".sms"))
        _case(out, name, m, n, ent, nseeds=FIXTURE_SEEDS.get(name, 64), fixture=os.path.join(DATA, name + ".sms"))
    for c in synth.cse_cases():
        if c.hbm or (c.family == "moduli" and c.p != PRIME0):
            continue
        _case(out, "q_" + c.name, c.m, c.n, mapped_entries(c))
    # columns 2 and 4 tie at -1 and at 1, columns 2 and 3 at 2 and at -2 ...: the tie list over Q and the one over residues differ in order
    rows = [{2: F(-1, 2), 3: F(-1), 4: F(1, 2)},
            {0: F(2), 2: F(-1, 2), 3: F(3), 4: F(-1, 2)},
            {1: F(3), 2: F(-1, 2), 3: F(-1, 3), 4: F(-1, 2)},
            {0: F(2), 1: F(-1, 3), 2: F(1, 2), 3: F(1), 4: F(-1, 2)}]
    _case(out, "tie_order", 4, 5, _rows_ent(rows))
    # row 1 holds 3/2 = 3 / 2, the quotient of its entry of column 0 by row 0's: Triangle fires on that couple; rows 4 and 2 have one
    # too, which the never-reset `found` skips (synth.cse_cases, triangle_found); the pivot of the second matrix is negative
    rows = [{0: 2, 1: 1}, {0: 3, 2: F(3, 2)}, {0: 5, 3: 1}, {0: 7, 4: 1}, {0: 11, 5: F(11, 5)}]
    _case(out, "triangle", 5, 6, _rows_ent(rows))
    _case(out, "triangle_neg", 3, 4, _rows_ent([{0: -2, 1: 5}, {0: 6, 2: 3}, {0: F(1, 2), 3: F(-1, 3)}]))
    # 8 rows over 8 columns with the values 2 .. 65, rows 0 .. 3 twice: 64 distinct values, steps of frequency 2
    base = [{j: 2 + 8 * i + j for j in range(8)} for i in range(8)]
    _case(out, "values64", 12, 8, _rows_ent(base + [dict(r) for r in base[:4]]))
    more = base + [dict(r) for r in base[:4]]
    more[11][7] = 66
    _case(out, "values65", 12, 8, _rows_ent(more), refused=UNSUPPORTED, why="65 distinct values")
    _case(out, "prime_step", 3, 2, _rows_ent([{0: 2 * PRIME0, 1: 1}, {0: 2 * PRIME0, 1: 1}, {0: 1, 1: 2}]))
    _case(out, "collide", 3, 2, _rows_ent([{0: 1, 1: 2 ** 30 + 4}, {0: 1, 1: 2 ** 30 + 4}, {0: 2, 1: 1}]))
    big = [F(2 ** 61 - 1, 2 ** 61 - 3), F(2 ** 61 - 5, 2 ** 61 - 9), F(2 ** 61 - 11, 2 ** 61 - 15), F(2 ** 61 - 17, 2 ** 61 - 21)]
    _case(out, "overflow", 2, 2, _rows_ent([{0: big[0], 1: big[1]}, {0: big[2], 1: big[3]}]), refused=UNSUPPORTED, why="128-bit overflow")
    return out


def running():
    return [c for c in cases() if not c.refused]


def goldens():
    """{case name: [(adds, muls) per seed]} of tests/golden/cse_q_costs.json"""
    import json
    from plo_testlib import GOLDEN
    with open(os.path.join(GOLDEN, "cse_q_costs.json")) as f:
        return {e["name"]: list(zip(e["adds"], e["muls"])) for e in json.load(f)["cases"]}


def is_prime(x):
    return x >= 2 and all(x % d for d in range(2, int(x ** 0.5) + 1))


def residue(v, p):
    """v modulo p, or None when p divides its numerator or its denominator"""
    if v.numerator % p == 0 or v.denominator % p == 0:
        return None
    return v.numerator % p * pow(v.denominator % p, -1, p) % p


def separates(U, p):
    res = [residue(v, p) for v in U]
    return None not in res and len(set(res)) == len(res)


def colliding_prime(U, limit=64):
    """the smallest prime of 31 bits (from 2^30 up, `limit` primes looked at) modulo which two elements of U have the same residue"""
    p, seen = 2 ** 30, 0
    while seen < limit:
        p += 1
        if not is_prime(p):
            continue
        seen += 1
        res = [residue(v, p) for v in U]
        if None not in res and len(set(res)) < len(res):
            return p
    return None


def prime_below(p):
    p -= 1
    while not is_prime(p):
        p -= 1
    return p
