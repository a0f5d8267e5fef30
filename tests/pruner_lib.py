"""What the tests of bin/pruner share: running the tool, reading its report, and an independent restatement of its window
rule over plo_testlib.tokenize_slp."""
import os
import re
import subprocess

from plo_testlib import ROOT, count_ops, eval_slp, tokenize_slp

PRUNER = os.path.join(ROOT, "bin", "pruner")
CHK = os.path.join(ROOT, "bin", "SLPchecker")
REPORT = re.compile(r"^(.+) \[(\d+)x(\d+)\]: (\d+)\|(\d+)(?: D (\d+)\|(\d+) \[seed (\d+)\])?(?: G (\d+)\|(\d+) \[seed (\d+)\])? (IMPROVEMENT|== less additions|== less multiplications|==|≤)$")


def build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "plinopt_amd", "csrc", "host")])


def run(args, stdin=None, tool=PRUNER):
    r = subprocess.run([tool] + [str(a) for a in args], input=stdin, capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def report(out):
    """the windows of a report: sel, dims, before, D and G as (adds, muls, seed) or None, mark, and the replacement's lines"""
    wins = []
    for line in out.splitlines():
        if ":=" in line:
            wins[-1]["repl"].append(line)
            continue
        g = REPORT.match(line)
        assert g, line
        num = lambda *ks: tuple(int(g.group(k)) for k in ks) if g.group(ks[0]) is not None else None   # noqa: E731
        wins.append(dict(sel=g.group(1).split(" "), dims=num(2, 3), before=num(4, 5), D=num(6, 7, 8), G=num(9, 10, 11), mark=g.group(12), repl=[]))
    return wins


def _isvar(t):
    return t[0].isalpha() or t[0] == "_"


def windows(text, singles, only=None):
    """The window rule, restated: per selection its body's lines, inputs (sorted), outputs (sorted downwards, without the
    first selected variable) and the operations of the body"""
    lines = tokenize_slp(text)
    lhs = [l[0] for l in lines]
    uses = [{t for t in l[2:] if _isvar(t)} for l in lines]
    names = [v for v in dict.fromkeys(lhs) if not v.startswith("o") and (only is None or v in only)]
    out = []
    for sel in ([(a,) for a in names] if singles else [(a, b) for a in names for b in names]):
        near = set(sel).union(*[uses[lhs.index(v)] for v in sel])
        body = [k for k in range(len(lines)) if lhs[k] in near or uses[k] & near]
        defined = {lhs[k] for k in body}
        ins = sorted(set().union(*[uses[k] for k in body]) - defined)
        outs = sorted(defined - {sel[0]}, reverse=True)
        if outs and sel[0] in defined:
            out.append(dict(sel=list(sel), body=["".join(lines[k]) for k in body], ins=ins, outs=outs, before=count_ops("\n".join("".join(lines[k]) for k in body))))
    return out


def renamed(lines, W):
    """program lines with the window's inputs as i# and its outputs as o# (eval_slp's names)"""
    nm = {v: "i%d" % k for k, v in enumerate(W["ins"])}
    nm.update({v: "o%d" % k for k, v in enumerate(W["outs"])})
    return "\n".join("".join(nm.get(t, t) for t in toks) for toks in tokenize_slp("\n".join(lines)))


def window_matrix(W, field):
    """{(row, column): coefficient} of a window: its outputs in terms of its inputs"""
    nm = {v: "i%d" % k for k, v in enumerate(W["ins"])}
    body = "\n".join("".join(nm.get(t, "w_" + t if _isvar(t) else t) for t in toks) for toks in tokenize_slp("\n".join(W["body"])))
    tail = "\n".join("o%d:=w_%s;" % (k, v) for k, v in enumerate(W["outs"]))
    return eval_slp(body + "\n" + tail, field)


def csr_of(mat, m, n):
    rp, c, v = [0], [], []
    for i in range(m):
        for j in range(n):
            if mat.get((i, j)):
                c.append(j)
                v.append(mat[(i, j)])
        rp.append(len(c))
    return m, n, rp, c, v
