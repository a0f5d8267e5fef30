"""Optimizer() of the reference (include/plinopt_optimize.inl:30-631), counts only, restated literally in Python over a field object.

Independent of the product code: the HIP kernels, the C API, the host tools and oracle/plo_oracle.c are not used here.  The one
convention taken from the project is the per-candidate random stream of include/plinopt_hip.h (the reference draws from a
thread-local GivRandom): candidate `seed` starts the GivRandom LCG at 1 + splitmix64(seed) mod (2^31 - 2).

Fields: QQ (fractions.Fraction, rational order and sign) and Zp (canonical residues, integer order, Fabs / Fsign of
include/plinopt_library.h:203-225).  Elements order by Python's `<`, which is what std::map<triple, size_t> and
std::map<Element, size_t> use in the reference.  A field with `seen = set()` records every value a candidate stores, forms
or compares: entries, pair ratios, inverses, absolute values and Triangle's quotients.
"""
from fractions import Fraction

M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


class CandRng:
    """GivRandom's generator, one stream per candidate"""

    def __init__(self, seed):
        self.s = 1 + splitmix64(seed) % 2147483646

    def next(self):
        self.s = 950706376 * self.s % 2147483647
        return self.s


class _Field:
    seen = None

    def rec(self, x):
        if self.seen is not None:
            self.seen.add(x)
        return x

    def abs_one(self, e):                       # isAbsOne, plinopt_library.h
        return e == self.one or e == self.mone

    def div(self, a, b):
        return self.rec(self._div(self.rec(a), self.rec(b)))

    def inv(self, a):
        return self.rec(self._div(self.one, self.rec(a)))

    def fabs(self, e):
        return self.rec(self._abs(self.rec(e)))


class QQ(_Field):
    name = "Q"
    one, mone = Fraction(1), Fraction(-1)

    def conv(self, fr):
        return Fraction(fr)

    def _div(self, a, b):
        return a / b

    def _abs(self, e):
        return abs(e)

    def sign(self, e):
        return (e > 0) - (e < 0)

    def mul_counts(self, e):                    # printmulorjustdiv, rational specialisation (plinopt_library.inl:360-374)
        return e != 1


class Zp(_Field):
    def __init__(self, p):
        self.p, self.name, self.one, self.mone = p, "Z/%dZ" % p, 1 % p, p - 1

    def conv(self, fr):
        fr = Fraction(fr)
        return fr.numerator % self.p * pow(fr.denominator % self.p, -1, self.p) % self.p

    def _div(self, a, b):
        return a * pow(b, -1, self.p) % self.p

    def _abs(self, e):                          # Fabs: a = -e; a < e ? a : e
        a = (self.p - e) % self.p
        return a if a < e else e

    def sign(self, e):                          # Fsign
        if e == 0:
            return 0
        return -1 if (self.p - e) % self.p < e else 1

    def mul_counts(self, e):                    # printmulorjustdiv, generic (plinopt_library.inl:347-358)
        return not self.abs_one(e)


def _transpose(rows, nout):
    T = [[] for _ in range(nout)]
    for i, row in enumerate(rows):
        for c, v in row:
            T[c].append((i, v))
    return T


class Optimizer:
    """One candidate: Optimizer(sout, M, ...) :616-631 on the rows [[(column, element), ...], ...] (columns ascending)."""

    def __init__(self, F, rows, ncols, seed):
        self.F, self.M, self.ncols, self.rng = F, [list(r) for r in rows], ncols, CandRng(seed)
        self.nbadd = self.nbmul = 0
        self.multiples = []                     # (index, column, value)
        self.triangles = 0                      # how often Triangle fired
        for r in self.M:
            for _, v in r:
                F.rec(v)

    def run(self):
        while self.one_sub():
            pass
        self.program_gen()
        return self.nbadd, self.nbmul

    # ---- :30-41
    def listpairs(self, row):
        return [(row[x][0], row[y][0], self.F.div(row[y][1], row[x][1])) for x in range(len(row)) for y in range(x + 1, len(row))]

    def find_mult(self, col, val):
        return any(c == col and v == val for _, c, v in self.multiples)

    # ---- :60-194
    def rem_one_cse(self, cse, AP, PM):
        F, lm = self.F, self.ncols
        c0 = sum(1 for r in self.M for c, v in r if c == cse[0] and F.abs_one(v))
        c1 = sum(1 for r in self.M for c, v in r if c == cse[1] and F.abs_one(v))
        l = (cse[1], cse[0], F.inv(cse[2])) if c0 < c1 else cse
        for i in range(len(AP)):
            ap = AP[i]
            if cse not in ap:
                continue
            row, coeff = self.M[i], None
            for k, (c, v) in enumerate(row):
                if c == l[0]:
                    coeff = v
                    del row[k]
                    break
            for k, (c, v) in enumerate(row):
                if c == l[1]:
                    del row[k]
                    row.append((lm, coeff))
                    break
            for t in ap:
                PM[t] -= 1
                if PM[t] == 0:
                    del PM[t]
            nr = [t for t in ap if t[0] != l[0] and t[1] != l[0] and t[0] != l[1] and t[1] != l[1]]
            last = row[-1]
            for c, v in row[:-1]:
                nr.append((c, last[0], F.div(last[1], v)))
            for t in nr:
                PM[t] = PM.get(t, 0) + 1
            AP[i] = nr
        asgs = F.fabs(l[2])
        if not F.abs_one(asgs):
            if not self.find_mult(l[1], asgs):
                self.nbmul += F.mul_counts(asgs)
                self.multiples.append((lm, l[1], asgs))
        self.ncols = lm + 1

    # ---- :209-314 (RANDOM_TIES)
    def one_sub(self):
        AP = [self.listpairs(row) for row in self.M]
        PM = {}
        for ap in AP:
            for t in ap:
                PM[t] = PM.get(t, 0) + 1
        if not PM:
            return False
        good = False
        while PM:
            maxfrq = max(PM.values())
            if maxfrq <= 1:
                return good
            good = True
            mx = sorted(t for t, f in PM.items() if f == maxfrq)             # std::map order of the triples
            cse = mx[0]
            if len(mx) > 1:
                cse = mx[self.rng.next() % len(mx)]
            self.nbadd += 1
            self.rem_one_cse(cse, AP, PM)
        return True

    def histo(self, row):
        h = {}
        for _, v in row:
            a = self.F.fabs(v)
            h[a] = h.get(a, 0) + 1
        return h

    # ---- :318-371
    def factor_out_columns(self, T, j):
        F = self.F
        if not T[j]:
            return
        h = self.histo(T[j])
        for e in sorted(h):
            m = len(T)
            if h[e] > 1 and not F.abs_one(e):
                if not self.find_mult(j, e):
                    self.nbmul += F.mul_counts(e)
                    self.multiples.append((m, j, e))
                T.append([])
                for _ in range(h[e]):
                    row = T[j]
                    for k, (c, v) in enumerate(row):
                        if F.fabs(v) == e:
                            T[m].append((c, F.one if F.sign(v) >= 0 else F.mone))
                            del row[k]
                            break

    # ---- :375-420
    def factor_out_rows(self, A, i):
        F = self.F
        if not A[i]:
            return
        h = self.histo(A[i])
        m = self.ncols
        for e in sorted(h):
            if h[e] > 1 and not F.abs_one(e):
                m += 1
                self.ncols = m
                row = A[i]
                row.append((m - 1, e))
                for k, (c, v) in enumerate(row):
                    if F.fabs(v) == e:
                        del row[k]
                        break
                for _ in range(1, h[e]):
                    for k, (c, v) in enumerate(row):
                        if F.fabs(v) == e:
                            self.nbadd += 1
                            del row[k]
                            break

    # ---- :427-507; works on self.M and self.T
    def triangle(self, j):
        F = self.F
        if not self.T[j]:
            return False
        found = False
        while True:
            over = True
            Tj = self.T[j]
            for it in range(len(Tj)):
                if F.abs_one(Tj[it][1]):
                    continue
                for nx in range(len(Tj)):
                    if nx == it or F.abs_one(Tj[nx][1]):
                        continue
                    iter_, next_ = Tj[it], Tj[nx]
                    i = next_[0]
                    quot = F.div(next_[1], iter_[1])
                    for c3, v3 in self.M[i]:
                        if c3 == j or F.abs_one(v3):
                            continue
                        # isAbsOne(quot / third): an equality test of quot against +-third, both recorded; the quotient of the two is not a
                        # value of the matrix and is not recorded
                        F.rec(v3)
                        if not F.abs_one(F._div(quot, v3)):
                            continue
                        m = len(self.T)
                        found, over = True, False
                        self.triangles += 1
                        self.nbmul += F.mul_counts(F.fabs(iter_[1]))
                        self.multiples.append((m, j, iter_[1]))
                        self.T.append([(iter_[0], F.one), (next_[0], quot)])
                        self.T[j] = [q for q in Tj if q != iter_ and q != next_]
                        self.M = _transpose(self.T, len(self.M))
                        self.ncols = len(self.T)
                        self.factor_out_rows(self.M, i)
                        self.T = _transpose(self.M, self.ncols)
                        break
                    if found:
                        break
                if found:
                    break
            if over:
                return found

    # ---- :513-611
    def program_gen(self):
        F = self.F
        T = _transpose(self.M, self.ncols)
        for j in range(self.ncols):
            self.factor_out_columns(T, j)
        self.M = _transpose(T, len(self.M))
        self.ncols = len(T)
        for i in range(len(self.M)):
            self.factor_out_rows(self.M, i)
        self.T = _transpose(self.M, self.ncols)
        j = 0
        while j < self.ncols:                   # M.coldim() is read again after every column
            self.triangle(j)
            j += 1
        for row in self.M:
            for k, (c, v) in enumerate(row):
                if k > 0:
                    self.nbadd += 1
                ais = F.fabs(v)
                if not self.find_mult(c, ais):
                    self.nbmul += F.mul_counts(ais)


def field_rows(F, m, ent):
    """rows of the field image of {(i, j): Fraction}; entries that vanish are dropped"""
    rows = [[] for _ in range(m)]
    for (i, j), v in sorted(ent.items()):
        e = F.conv(v)
        if e != 0:
            rows[i].append((j, e))
    return rows


def cost(F, m, n, ent, seed):
    return Optimizer(F, field_rows(F, m, ent), n, seed).run()
