"""Literal restatement of the reference's `dependency` (src/dependency.cpp:44-170) with fractions.Fraction: the coefficient
list, the depth-first enumeration and the text it prints.  Test infrastructure: it shares nothing with
plinopt_amd/csrc/host/plo_dep.hpp, which it is there to check.

Stated readings: the matrix is walked row by row, columns ascending (`IndexedBegin`); over Z_q every value
is the residue in [0, q) and the `i` term prints Fsign/Fabs of that residue; a coefficient whose denominator is no unit
modulo q has no image and is dropped; a matrix entry with such a denominator is an error; `-l 0` is every depth."""
from fractions import Fraction

EVERY_DEPTH = (1 << 64) - 1


def parse_sms(text):
    """(m, n, rows): rows[i] = [(col, Fraction)] with columns ascending, zero entries dropped"""
    lines = [ln.split() for ln in text.splitlines() if ln.strip() and ln.strip()[0] not in "#%"]
    m, n = int(lines[0][0]), int(lines[0][1])
    rows = [dict() for _ in range(m)]
    for t in lines[1:]:
        i, j = int(t[0]), int(t[1])
        if i == 0 and j == 0:
            break
        v = Fraction(t[2])
        if v != 0:
            rows[i - 1][j - 1] = v
    return m, n, [sorted(r.items()) for r in rows]


def load_sms(path):
    with open(path) as f:
        return parse_sms(f.read())


def to_sms(m, n, rows):
    out = ["%d %d R" % (m, n)]
    for i, r in enumerate(rows):
        for j, v in r:
            out.append("%d %d %s" % (i + 1, j + 1, v))
    out.append("0 0 0")
    return "\n".join(out) + "\n"


class QQ:
    zero, one = Fraction(0), Fraction(1)

    def image(self, r):
        return Fraction(r)

    def add(self, a, b):
        return a + b

    def sub(self, a, b):
        return a - b

    def mul(self, a, b):
        return a * b

    def neg(self, a):
        return -a

    def show(self, letter, idx, r):                       # showOut, :52-63
        s = ("-" if r < 0 else "+") + letter + str(idx)
        if r != 1 and r != -1:
            if abs(r.numerator) == 1:
                s += "/" + str(r.denominator)
            else:
                s += "*" + str(abs(r))
        return s

    def text(self, r):
        return str(r)


class Zq:
    def __init__(self, q):
        self.q, self.zero, self.one = q, 0, 1 % q

    def image(self, r):
        """residue of the rational r, or None when its denominator is no unit modulo q"""
        r = Fraction(r)
        try:
            inv = pow(r.denominator % self.q, -1, self.q)
        except ValueError:
            return None
        return r.numerator * inv % self.q

    def add(self, a, b):
        return (a + b) % self.q

    def sub(self, a, b):
        return (a - b) % self.q

    def mul(self, a, b):
        return a * b % self.q

    def neg(self, a):
        return (-a) % self.q

    def show(self, letter, idx, e):                       # showOut :44-50 with Fsign/Fabs, plinopt_library.h:208-225
        a = self.neg(e)
        s = ("-" if (e != 0 and a < e) else "+") + letter + str(idx)
        if e != self.one and e != self.q - 1:
            s += "*" + str(a if a < e else e)
        return s

    def text(self, e):
        return str(e)


def field(q):
    return Zq(q) if q else QQ()


def rational_coefficients(rows, extra, maxnum):
    """:129-140 -- {1, -1}, the -v values, then r, -r, 1/r, -1/r for every numerator and denominator not yet listed, then for
    2, 3, ... while the list is short, truncated to maxnum"""
    C = [Fraction(1), Fraction(-1)] + [Fraction(x) for x in extra]

    def augment(r):
        if r not in C:
            C.extend([r, -r, 1 / r, -1 / r])
    for row in rows:
        for _, x in row:
            augment(Fraction(x.numerator))
            augment(Fraction(x.denominator))
    i = 2
    while len(C) < maxnum:
        augment(Fraction(i))
        i += 1
    del C[maxnum:]
    return C


def field_coefficients(F, C):
    """:142-151 -- images in list order, zeros, repeats (and values without an image) dropped"""
    FC = []
    for e in C:
        x = F.image(e)
        if x is not None and x != F.zero and x not in FC:
            FC.append(x)
    return FC


class BadDenominator(ValueError):
    pass


def field_matrix(F, rows):
    out = []
    for row in rows:
        r = []
        for j, x in row:
            y = F.image(x)
            if y is None:
                raise BadDenominator("denominator %d is no unit" % x.denominator)
            if y != F.zero:
                r.append((j, y))
        out.append(r)
    return out


def depender(m, n, rows, level=4, maxnum=11, extra=(), q=0, fc=None):
    """Returns (coefficient line, hits); a hit is (rows, coefficient indices, kind, column, -W[column], line): kind 0 is a
    vanishing combination, kind 1 one with a single non-zero; the indices are into FCoeffs (None for the top row).
    fc: a caller's FCoeffs (field elements) in place of the list of :129-151."""
    F = field(q)
    M = field_matrix(F, rows)
    FC = list(fc) if fc is not None else field_coefficients(F, rational_coefficients(rows, extra, maxnum))
    head = "# [DEPND] level %d, coefficients: [%s]" % (level, ",".join(F.text(c) for c in FC))
    hits = []
    LC, IX = [], []
    W = [F.zero] * n

    def show_lc():
        return "".join(F.show("o", r, c) for r, c in LC) + ";"

    def explore(last, lvl):                               # :74-101
        if lvl <= 0:
            return
        for qq in range(last + 1, m):
            prevv = F.zero
            for v in range(len(FC)):
                currv = F.sub(FC[v], prevv)
                prevv = FC[v]
                LC.append((qq, prevv)); IX.append(v)
                for j, x in M[qq]:
                    W[j] = F.add(W[j], F.mul(currv, x))
                nz = [j for j in range(n) if W[j] != F.zero]
                if not nz:
                    hits.append((tuple(r for r, _ in LC), tuple(IX), 0, 0, F.zero, show_lc()))
                elif len(nz) == 1:
                    j = nz[0]
                    hits.append((tuple(r for r, _ in LC), tuple(IX), 1, j, F.neg(W[j]), F.show("i", j, F.neg(W[j])) + show_lc()))
                explore(qq, lvl - 1)
                LC.pop(); IX.pop()
            for j, x in M[qq]:
                W[j] = F.sub(W[j], F.mul(prevv, x))

    lvl = level - 1 if level > 0 else EVERY_DEPTH
    for i in range(m):                                    # :158-165
        LC.append((i, F.one)); IX.append(None)
        for j, x in M[i]:
            W[j] = x
        explore(i, lvl)
        for j, _ in M[i]:
            W[j] = F.zero
        LC.pop(); IX.pop()
    return head, hits


def text_of(hits):
    return "".join(h[5] + "\n" for h in hits)


def combination(F, M, n, FC, hit_rows, hit_idx):
    """W of one combination, dense: what a caller recomputes from a device hit"""
    W = [F.zero] * n
    for r, ix in zip(hit_rows, hit_idx):
        c = F.one if ix is None else FC[ix]
        for j, x in M[r]:
            W[j] = F.add(W[j], F.mul(c, x))
    return W


def line_of(F, FC, hit_rows, hit_idx, W):
    """the reference's line for a combination whose value is W, or None when it is no hit"""
    nz = [j for j, x in enumerate(W) if x != F.zero]
    if len(nz) > 1:
        return None
    lc = "".join(F.show("o", r, F.one if ix is None else FC[ix]) for r, ix in zip(hit_rows, hit_idx)) + ";"
    return lc if not nz else F.show("i", nz[0], F.neg(W[nz[0]])) + lc
