"""The independent definition of what bin/TPchecker certifies, and the cases its tests run.

The definition reads the program text with its own regular expressions and evaluates it on symbolic linear forms over Fraction:
A, B, C (the final a, b, c as combinations of the inputs) and S (per slot of c, the coefficient of every a_i b_j; with -e the low
slots, then the hig ones).  Modulo q the rational values are reduced at the end, which is the same map as computing modulo q
when every denominator is a unit (otherwise the definition refuses, as the tool must).  It returns (violated, first, found,
expected) under the equation numbering of DESIGN.md 2.14:
    e = (i nb + j) w + z,  then A: E0 + x na + i,  then nb^2 numbers for B,  then nc^2 for C.

The cases: synthetic schoolbook triples (products t = (i, j), L[t][i] = R[t][j] = P[i+j][t] = 1) whose program the generator
writes itself, all AXPYs with add/undo and scale/unscale lines around them on all three families; mutations of such a program;
and a defect that the first certificate prime hides."""
import math
import os
import re
import subprocess
from fractions import Fraction

from plo_testlib import ROOT, csr_rational

TPC = os.path.join(ROOT, "bin", "TPchecker")
ANSI = re.compile(r"\x1b\[[0-9;]*m")
P31 = 2147483629                     # the first certificate prime
P62 = 4611686018427387847            # a 62-bit prime (2^62 - 57)
ADD, SCA, AXPY = 0, 1, 2


class Refused(Exception):
    """what the tool must refuse with exit status 4: (line number or None, kind); KINDS maps the kind to words of the reason"""

    def __init__(self, line, kind):
        super().__init__("line %s: %s" % (line, kind))
        self.line, self.kind = line, kind


KINDS = {
    "grammar": None, "semicolon": "no ';'", "range": "index out of range", "first": "the destination is not the first operand",
    "families": "mixes families", "zero": "division by zero", "lowhig": "without -e", "plain": "without *low or *hig under -e",
    "unit": "is not invertible modulo",
}

_V = r"(-?\d+(?:/\d+)?)"
_X = r"([a-z])(\d+)"
_SCA = re.compile(r"^(-?)" + _X + r"(?:([*/])" + _V + r")?$")
_EAX = re.compile(r"^" + _X + r"([+-])\(" + _X + r"\*" + _X + r"\)\*(low|hig)$")
_AX = re.compile(r"^" + _X + r"([+-])" + _X + r"\*" + _X + r"$")
_ADD = re.compile(r"^" + _X + r"([+-])" + _X + r"(?:([*/])" + _V + r")?$")


def parse(text, na, nb, nc, expanded):
    """-> [(family, op, part, dst, src, src2, coefficient, line number)]; raises Refused"""
    dims = {"a": na, "b": nb, "c": nc}
    out = []

    def var(ln, letter, idx):
        if letter not in dims:
            raise Refused(ln, "grammar")
        if int(idx) >= dims[letter]:
            raise Refused(ln, "range")
        return "abc".index(letter), int(idx)

    def factor(ln, op, v):
        if op is None:
            return Fraction(1)
        num, _, den = v.partition("/")
        if den and int(den) == 0:
            raise Refused(ln, "zero")
        f = Fraction(int(num), int(den or 1))
        if op == "/":
            if f == 0:
                raise Refused(ln, "zero")
            f = 1 / f
        return f

    for ln, raw in enumerate(text.splitlines(), 1):
        line = raw.strip()
        if not line or line.startswith("#"):
            continue
        stmt = "".join(line.split(";")[0].split())
        if ":=" not in stmt:
            continue
        if ";" not in line:
            raise Refused(ln, "semicolon")
        lhs, rhs = stmt.split(":=", 1)
        md = re.match("^" + _X + "$", lhs)
        if not md:
            raise Refused(ln, "grammar")
        fam, dst = var(ln, *md.groups())
        m = _SCA.match(rhs)
        if m and (m.group(1) or m.group(4)):
            if var(ln, m.group(2), m.group(3)) != (fam, dst):
                raise Refused(ln, "first")
            f = factor(ln, m.group(4), m.group(5))
            out.append((fam, SCA, 0, dst, 0, 0, -f if m.group(1) else f, ln))
            continue
        m = _EAX.match(rhs) or _AX.match(rhs)
        if m:
            if var(ln, m.group(1), m.group(2)) != (fam, dst):
                raise Refused(ln, "first")
            (fa, ia), (fb, ib) = var(ln, m.group(4), m.group(5)), var(ln, m.group(6), m.group(7))
            half = m.group(8) if m.re is _EAX else None
            if half and not expanded:
                raise Refused(ln, "lowhig")
            if (fam, fa, fb) != (2, 0, 1):
                raise Refused(ln, "families")
            if not half and expanded:
                raise Refused(ln, "plain")
            out.append((2, AXPY, {None: 0, "low": 1, "hig": 2}[half], dst, ia, ib, Fraction(-1 if m.group(3) == "-" else 1), ln))
            continue
        m = _ADD.match(rhs)
        if m:
            if var(ln, m.group(1), m.group(2)) != (fam, dst):
                raise Refused(ln, "first")
            f2, src = var(ln, m.group(4), m.group(5))
            if f2 != fam:
                raise Refused(ln, "families")
            f = factor(ln, m.group(6), m.group(7))
            out.append((fam, ADD, 0, dst, src, 0, -f if m.group(3) == "-" else f, ln))
            continue
        m = re.match("^-?" + _X, rhs)
        if m and var(ln, m.group(1), m.group(2)) != (fam, dst):
            raise Refused(ln, "first")
        raise Refused(ln, "grammar")
    return out


class Case:
    """A triple (each matrix (rows, columns, {(i, j): Fraction})), a program text and the two flags"""

    def __init__(self, name, L, R, P, text, expanded=False, matmul=False):
        self.name, self.L, self.R, self.P, self.text, self.expanded, self.matmul = name, L, R, P, text, expanded, matmul
        self.na, self.nb, self.nc0 = L[1], R[1], P[0]
        self.nc = self.nc0 + (1 if expanded else 0)
        self.w = 2 * self.nc if expanded else self.nc
        self.E0 = self.na * self.nb * self.w
        self.nequations = self.E0 + self.na ** 2 + self.nb ** 2 + self.nc ** 2
        self._defects = None

    def with_text(self, name, text):
        return Case(name, self.L, self.R, self.P, text, self.expanded, self.matmul)

    def flags(self):
        return (["-e"] if self.expanded else []) + (["-m"] if self.matmul else [])

    def records(self):
        """the records of the ctypes mirror"""
        return [(fam, op, part, dst, src, src2, co.numerator, co.denominator) for fam, op, part, dst, src, src2, co, _ in parse(self.text, self.na, self.nb, self.nc, self.expanded)]

    def csr(self):
        return [(m, n) + tuple(csr_rational(m, n, ent)) for m, n, ent in (self.L, self.R, self.P)]

    def write(self, d):
        """the three .sms files and the program in directory d -> the four paths"""
        paths = []
        for tag, (m, n, ent) in zip("LRP", (self.L, self.R, self.P)):
            paths.append(os.path.join(str(d), "%s_%s.sms" % (self.name, tag)))
            with open(paths[-1], "w") as f:
                f.write("%d %d R\n" % (m, n))
                for (i, j), v in sorted(ent.items()):
                    f.write("%d %d %s\n" % (i + 1, j + 1, v))
                f.write("0 0 0\n")
        paths.append(os.path.join(str(d), self.name + ".prog"))
        with open(paths[-1], "w") as f:
            f.write(self.text)
        return paths

    def where(self, e):
        """the tool's words for equation e"""
        if e < self.E0:
            pr, z = divmod(e, self.w)
            i, j = divmod(pr, self.nb)
            if not self.expanded:
                return "bilinear (i,j,z) = (%d,%d,%d)" % (i, j, z)
            return "bilinear (i,j,z) = (%d,%d,%d) %s" % (i, j, z % self.nc, "low" if z < self.nc else "hig")
        e -= self.E0
        for tag, n in zip("abc", (self.na, self.nb, self.nc)):
            if e < n * n:
                return "restoration of %s: %s[%d][%d]" % (tag, tag.upper(), e // n, e % n)
            e -= n * n
        raise ValueError(e)


def target(case):
    """{(i, j, z): T} without zeros"""
    T = {}
    if case.matmul:
        n = math.isqrt(case.nb * case.nc0 // case.na)
        m, k = case.nc0 // n, case.nb // n
        assert (m * k, k * n, m * n) == (case.na, case.nb, case.nc0)
        for a in range(m):
            for b in range(k):
                for c in range(n):
                    T[(a * k + b, b * n + c, a * n + c)] = Fraction(1)
        return T
    rows = {}
    for which, (_, _, ent) in enumerate((case.L, case.R)):
        for (t, x), v in ent.items():
            rows.setdefault(t, ([], [], []))[which].append((x, v))
    for (z, t), v in case.P[2].items():
        rows.setdefault(t, ([], [], []))[2].append((z, v))
    for ls, rs, ps in rows.values():
        for i, lv in ls:
            for j, rv in rs:
                for z, pv in ps:
                    T[(i, j, z)] = T.get((i, j, z), 0) + lv * rv * pv
    return {k: v for k, v in T.items() if v != 0}


def defects(case):
    """{e: (found, expected)} over Q for every equation with found != expected; raises Refused"""
    if case._defects is not None:
        return case._defects
    na, nb, nc, w = case.na, case.nb, case.nc, case.w
    recs = parse(case.text, na, nb, nc, case.expanded)
    lin = [[{x: Fraction(1)} for x in range(n)] for n in (na, nb, nc)]      # A, B, C: the rows are linear forms in the inputs
    S = [dict() for _ in range(w)]

    def axpy_into(dst, f, src):
        for k, v in src.items():
            nv = dst.get(k, 0) + f * v
            if nv:
                dst[k] = nv
            else:
                dst.pop(k, None)

    for fam, op, part, dst, src, src2, co, _ in recs:
        if op == AXPY:
            prod = {(i, j): va * vb for i, va in lin[0][src].items() for j, vb in lin[1][src2].items()}
            axpy_into(S[dst + (nc if part == 2 else 0)], co, prod)
            continue
        places = [(lin[fam], dst, src)]
        if fam == 2:
            places += [(S, dst + h, src + h) for h in ((0, nc) if case.expanded else (0,))]
        for F, d, sr in places:
            if op == SCA:
                F[d] = {k: v * co for k, v in F[d].items() if v * co}
            else:
                axpy_into(F[d], co, dict(F[sr]))
    out = {}
    want = {}
    for (i, j, z), v in target(case).items():
        if not case.expanded:
            want[(i * nb + j) * w + z] = v
        else:
            want[(i * nb + j) * w + z] = v
            want[(i * nb + j) * w + nc + z + 1] = v
    for z in range(w):
        for (i, j), v in S[z].items():
            e = (i * nb + j) * w + z
            if want.get(e, 0) != v:
                out[e] = (v, want.get(e, Fraction(0)))
    for e, v in want.items():
        z = e % w
        i, j = divmod(e // w, nb)
        if (i, j) not in S[z]:
            out[e] = (Fraction(0), v)
    e0 = case.E0
    for fam, n in enumerate((na, nb, nc)):
        for x in range(n):
            for i in set(lin[fam][x]) | {x}:
                v = lin[fam][x].get(i, Fraction(0))
                if v != (1 if x == i else 0):
                    out[e0 + x * n + i] = (v, Fraction(1 if x == i else 0))
        e0 += n * n
    case._defects = out
    return out


def denominators(case):
    ds = [co.denominator for *_, co, _ in parse(case.text, case.na, case.nb, case.nc, case.expanded)]
    lines = [ln for *_, ln in parse(case.text, case.na, case.nb, case.nc, case.expanded)]
    return list(zip(ds, lines)), ([] if case.matmul else [v.denominator for M in (case.L, case.R, case.P) for v in M[2].values()])


def definition(case, q=0, pair0=0, pair1=None):
    """(violated, first, found, expected), first None when nothing is violated; over Z/qZ the two values are residues"""
    pair1 = case.na * case.nb if pair1 is None else pair1
    prog, trip = denominators(case)
    if q:
        for d in trip:
            if math.gcd(d, q) != 1:
                raise Refused(None, "unit")
        for d, ln in prog:
            if math.gcd(d, q) != 1:
                raise Refused(ln, "unit")
    red = (lambda v: v) if not q else (lambda v: v.numerator * pow(v.denominator, -1, q) % q)
    bad = []
    for e, (got, exp) in defects(case).items():
        if e < case.E0:
            if not pair0 <= e // case.w < pair1:
                continue
        elif pair0 != 0:
            continue
        g, x = red(got), red(exp)
        if g != x:
            bad.append((e, g, x))
    if not bad:
        return 0, None, None, None
    first = min(bad)
    return (len(bad),) + first


def nequations(case, pair0=0, pair1=None):
    pair1 = case.na * case.nb if pair1 is None else pair1
    return (pair1 - pair0) * case.w + (case.nequations - case.E0 if pair0 == 0 else 0)


# ----------------------------------------------------------------------------- the certificate, in exact integers
def certificate(case):
    """(beta, j) of the rule of DESIGN.md 2.14: mu per variable, Delta the product of the lines' denominators, delta_T by the rule of the
    Brent certificate; beta = max(bits(mu) + bits(delta_T), bT) + bits(Delta) + 1 with the bits of a product taken as the sum of
    the bits of its factors."""
    recs = parse(case.text, case.na, case.nb, case.nc, case.expanded)
    mu = [[Fraction(1)] * n for n in (case.na, case.nb, case.nc)]
    dbits = 0
    for fam, op, part, dst, src, src2, co, _ in recs:
        if co.denominator > 1:
            dbits += co.denominator.bit_length()
        if op == AXPY:
            mu[2][dst] += mu[0][src] * mu[1][src2]
        elif op == SCA:
            mu[fam][dst] *= abs(co)
        else:
            mu[fam][dst] += abs(co) * mu[fam][src]
    top = max(max(v) for v in mu)
    bmu = max(1, (top.numerator // top.denominator).bit_length())
    bT, dT = 1, 0
    if not case.matmul:
        bT = case.L[0].bit_length()
        for _, _, ent in (case.L, case.R, case.P):
            bT += max([abs(v.numerator).bit_length() for v in ent.values()] or [0])
            d = sum(x.bit_length() for x in {v.denominator for v in ent.values()} if x > 1)
            bT += d
            dT += d
    beta = max(bmu + dT, bT) + dbits + 1
    return beta, (beta + 29) // 30


def cleared_defect_bits(case):
    """the bits of the largest |found - expected| Delta delta_T"""
    prog, trip = denominators(case)
    delta = 1
    for d, _ in prog:
        delta *= d
    for d in set(trip):
        delta *= d
    worst = 0
    for got, exp in defects(case).values():
        v = abs(got - exp) * delta
        assert v.denominator == 1
        worst = max(worst, v.numerator.bit_length())
    return worst


# ----------------------------------------------------------------------------- the generator
FLAVOURS = {"issue": (3, Fraction(-5, 3)), "units": (7, Fraction(-7, 4))}     # "units": every denominator is a unit modulo 3 and 15


def schoolbook(na, nb, expanded=False, flavour="issue", name=None):
    k1, f2 = FLAVOURS[flavour]
    f2t, f2u = "*%s" % f2, "*%s" % (1 / f2)
    nc0 = na + nb - 1
    nc = nc0 + (1 if expanded else 0)
    one = Fraction(1)
    L = (na * nb, na, {(i * nb + j, i): one for i in range(na) for j in range(nb)})
    R = (na * nb, nb, {(i * nb + j, j): one for i in range(na) for j in range(nb)})
    P = (nc0, na * nb, {(i + j, i * nb + j): one for i in range(na) for j in range(nb)})
    out = []

    def axpy(K, i, j, sign="+"):
        if expanded:
            return ["c%d:=c%d %s (a%d * b%d)*low; ### AXPY low  ###" % (K, K, sign, i, j), "c%d:=c%d %s (a%d * b%d)*hig; ### AXPY high ###" % (K + 1, K + 1, sign, i, j)]
        return ["c%d:=c%d %s a%d * b%d; ### AXPY ###" % (K, K, sign, i, j)]

    def on_c(K, what):
        """a scaling of the entries of c that the AXPY into K meets"""
        return [("c%d:=" + what + ";") % (K + d, K + d) for d in range(2 if expanded else 1)]

    if nc >= 2:
        out += ["# generated", "c0:=c0+c1*%d;" % k1, "c0:=c0-c1*%d;" % k1]
    for i in range(na):
        for j in range(nb):
            K = i + j
            pat = (i * nb + j) % 8
            k, l = (i + 1) % na, (j + 1) % nb
            free = [M for M in range(nc) if M not in (K, K + 1)] if expanded else [M for M in range(nc) if M != K]
            if pat == 1:
                out += ["a%d:=a%d*%d;" % (i, i, k1)] + on_c(K, "c%%d*%d" % k1) + axpy(K, i, j) + on_c(K, "c%%d/%d" % k1) + ["a%d:=a%d/%d;" % (i, i, k1)]
            elif pat == 2 and na >= 2:
                out += ["a%d:=a%d+a%d*%d;" % (i, i, k, k1)] + axpy(K, i, j) + ["a%d:=a%d-a%d*%d;" % (i, i, k, k1)]
                out += ["a%d:=a%d*%d;" % (k, k, k1)] + axpy(K, k, j, "-") + ["a%d:=a%d/%d;" % (k, k, k1)]
            elif pat == 3:
                out += ["b%d:=b%d%s;" % (j, j, f2t)] + on_c(K, "c%%d%s" % f2t) + axpy(K, i, j) + on_c(K, "c%%d%s" % f2u) + ["b%d:=b%d%s;" % (j, j, f2u)]
            elif pat == 4:
                out += ["b%d:=-b%d/2;" % (j, j)] + on_c(K, "-c%d/2") + axpy(K, i, j) + on_c(K, "-c%d*2") + ["b%d:=-b%d*2;" % (j, j)]
            elif pat == 5 and free:
                M = free[(i + j) % len(free)]
                out += ["c%d:=c%d+c%d/2;" % (K, K, M)] + axpy(K, i, j) + ["c%d:=c%d-c%d/2;" % (K, K, M)]
            elif pat == 6 and nb >= 2:
                out += ["b%d:=b%d-b%d/2;" % (j, j, l)] + axpy(K, i, j) + ["b%d:=b%d+b%d/2;" % (j, j, l)]
                out += on_c(K, "c%d*2") + axpy(K, i, l) + on_c(K, "c%d/2")
            elif pat == 7 and na >= 2:
                out += ["a%d:=a%d+a%d*%d;" % (i, i, k, k1), "a%d:=a%d-a%d*%d;" % (i, i, k, k1)] + axpy(K, i, j)
            else:
                out += axpy(K, i, j)
    name = name or "school_%dx%d%s_%s" % (na, nb, "e" if expanded else "", flavour)
    return Case(name, L, R, P, "\n".join(out) + "\n", expanded)


def edge_cases(flavour="issue"):
    out = []
    for expanded in (False, True):
        out += [schoolbook(2, nb, expanded, flavour) for nb in (1, 63, 64, 65, 129)] + [schoolbook(1, 5, expanded, flavour)]
    return out


def limit_cases(max_words):
    """(at the limit, one above), plain and with -e: na = 1, so that w = nb or 2 (nb + 1)"""
    return [(schoolbook(1, max_words), schoolbook(1, max_words + 1)), (schoolbook(1, max_words // 2 - 1, True), schoolbook(1, max_words // 2, True))]


def mutations(base=None):
    """[(Case, blocks)]: blocks names the blocks (0 bilinear, 1 A, 2 B, 3 C) that must hold a violated equation"""
    base = base or schoolbook(3, 5)
    lines = base.text.splitlines()

    def edit(name, pick, change, blocks):
        idx = [n for n, ln in enumerate(lines) if pick(ln)]
        assert idx, name
        n = idx[-1] if name.startswith("last") or name.startswith("restore") or name == "both" else idx[len(idx) // 2]
        new = lines[:n] + change(lines[n]) + lines[n + 1:]
        return base.with_text(base.name + "_" + name, "\n".join(new) + "\n"), blocks

    is_ax = lambda ln: " * " in ln
    out = [
        edit("dropped", is_ax, lambda ln: [], {0}),
        edit("sign", is_ax, lambda ln: [ln.replace(" + ", " - ", 1) if " + " in ln else ln.replace(" - ", " + ", 1)], {0}),
        edit("coefficient", lambda ln: re.match(r"^c\d+:=c\d+/\d+;", ln), lambda ln: [re.sub(r"/(\d+);", lambda m: "/%d;" % (int(m.group(1)) + 1), ln)], {0}),
        edit("swapped", lambda ln: re.search(r"a(\d+) \* b(\d+)", ln) and len(set(re.search(r"a(\d+) \* b(\d+)", ln).groups())) == 2 and max(map(int, re.search(r"a(\d+) \* b(\d+)", ln).groups())) < min(base.na, base.nb),
             lambda ln: [re.sub(r"a(\d+) \* b(\d+)", r"a\2 * b\1", ln)], {0}),
        edit("wrongc", is_ax, lambda ln: [re.sub(r"c(\d+)", lambda m: "c%d" % ((int(m.group(1)) + 1) % base.nc), ln)], {0}),
        edit("restore_a", lambda ln: re.match(r"^a\d+:=a\d+/\d+;", ln), lambda ln: [], {1}),
        edit("restore_b", lambda ln: re.match(r"^b\d+:=-b\d+\*2;", ln), lambda ln: [], {2}),
        edit("restore_c", lambda ln: re.match(r"^c0:=c0-c1\*\d+;", ln), lambda ln: [], {3}),
        edit("both", lambda ln: re.match(r"^c\d+:=c\d+/\d+;", ln), lambda ln: [], {0, 3}),
    ]
    return out


def hidden_defect(base=None):
    """c0 gets p1 c1 and keeps it: invisible modulo the first certificate prime"""
    base = base or schoolbook(2, 3)
    return base.with_text(base.name + "_hidden", "c0:=c0+c1*%d;\n" % P31 + base.text)


# lines outside the grammar, as line 3 of a program for na = 2, nb = 3, nc = 4 without -e, and the kind of each refusal
REFUSED = [
    ("c0:=c0+a1;", "families"), ("a0:=a0+b0*3;", "families"), ("c0:=c0 + b0 * a0;", "families"), ("a0:=a0 + a0 * b0;", "families"),
    ("a2:=a2*3;", "range"), ("c0:=c0+c9;", "range"), ("c0:=c0 + a0 * b7;", "range"),
    ("a0:=a1+a0;", "first"), ("c1:=c0 + a0 * b0;", "first"), ("a0:=-a1;", "first"),
    ("a0:=a0/0;", "zero"), ("a0:=a0+a1/0;", "zero"), ("a0:=a0*1/0;", "zero"),
    ("c0:=c0 + (a0 * b0)*low;", "lowhig"), ("c1:=c1 - (a0 * b0)*hig;", "lowhig"),
    ("a0:=a0;", "grammar"), ("a0:=a0+a1+a1;", "grammar"), ("x0:=x0*3;", "grammar"), ("a0:=a0*x;", "grammar"), ("a0:=a0+a1*3", "semicolon"),
]


# ----------------------------------------------------------------------------- the tool
def tool(args, gpu=0, stdin=None, env=None, timeout=300, exe=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([exe or TPC] + ([] if gpu is None else ["--gpu", str(gpu)]) + [str(a) for a in args], input=stdin, capture_output=True, text=True, timeout=timeout, env=e)
    return r.returncode, ANSI.sub("", r.stderr)


def first_of(err):
    """(e, where, found text, expected text) of the `# first violated equation` line"""
    mt = re.search(r"# first violated equation e=(\d+): (.*?), found (\S+) instead of ([^\s;]+)", err)
    assert mt, err
    return int(mt.group(1)), mt.group(2), mt.group(3), mt.group(4)


def count_of(err):
    mt = re.search(r"# (\d+) of (\d+) equations violated", err)
    assert mt, err
    return int(mt.group(1)), int(mt.group(2))


def cert_of(err):
    mt = re.search(r"# certificate: beta = (\d+), j = (\d+), primes((?: \d+)+)", err)
    assert mt, err
    return int(mt.group(1)), int(mt.group(2)), [int(x) for x in mt.group(3).split()]


def passes_of(err):
    return [(int(a), int(b), int(p), t) for a, b, p, t in re.findall(r"# pass (\d+) of (\d+) modulo (\d+): (no violated equation|violated)", err)]
