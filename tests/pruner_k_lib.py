"""What the tests of bin/pruner -K share on top of tests/pruner_lib.py: the report with its K group between D and G, and the
oracle's kernel-method minimum of a window."""
import re

import pruner_lib as pl
from pruner_lib import renamed, window_matrix, windows, csr_of, run  # noqa: F401  (re-exported for the tests)

_GROUP = r"(?: %s (\d+)\|(\d+) \[seed (\d+)\])?"
REPORT = re.compile(r"^(.+) \[(\d+)x(\d+)\]: (\d+)\|(\d+)" + _GROUP % "D" + _GROUP % "K" + _GROUP % "G" + r" (IMPROVEMENT|== less additions|== less multiplications|==|≤)$")


def report(out):
    """pruner_lib.report with the K group: sel, dims, before, D, K and G as (adds, muls, seed) or None, mark, replacement lines"""
    wins = []
    for line in out.splitlines():
        if ":=" in line:
            wins[-1]["repl"].append(line)
            continue
        g = REPORT.match(line)
        assert g, line
        num = lambda *ks: tuple(int(g.group(k)) for k in ks) if g.group(ks[0]) is not None else None   # noqa: E731
        wins.append(dict(sel=g.group(1).split(" "), dims=num(2, 3), before=num(4, 5), D=num(6, 7, 8), K=num(9, 10, 11), G=num(12, 13, 14), mark=g.group(15), repl=[]))
    return wins


def best_of(g):
    """(method, (adds, muls)) of a report line: best of D, K, G under cmpOpCount, the earlier method winning ties; None without a result"""
    have = [(k, g[k][:2]) for k in "DKG" if g[k]]
    return min(have, key=lambda kv: (sum(kv[1]), kv[1][0], "DKG".index(kv[0]))) if have else None


def mark_of(g):
    """the first word of the mark that the best result earns (mirabelle.sh:139-175)"""
    dif = sum(g["before"]) - sum(best_of(g)[1])
    return "IMPROVEMENT" if dif > 0 else "==" if dif == 0 else "≤"


def kernel_min(O, seed0, n):
    """(adds, muls, seed) of the minimum of O.kernel_restart over seed0 .. seed0+n-1 under (sum, adds, seed); None: no kernel"""
    if O.kernel_restart(seed0) is None:
        return None
    r = [O.kernel_restart(s)[:2] for s in range(seed0, seed0 + n)]
    j = min(range(n), key=lambda j: (sum(r[j]), r[j][0], j))
    return r[j] + (seed0 + j,)


def defined_once(lines):
    lhs = [l.split(":=")[0] for l in lines]
    return len(lhs) == len(set(lhs))
