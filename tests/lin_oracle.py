"""Literal Python restatement of the reference's in-place linear search (bin/inplacer), over Fraction.

Independent of plinopt_amd/csrc/host/plo_inplace.hpp: it is what the host tool, the HIP kernel (plo_lin.hip) and
tests/golden/lin_costs.json are held to.  Line numbers are those of the reference:
  include/plinopt_inplace.inl   Atom :15-124, complexity :133-144, Pprint :163-175, orientindex :179-216,
                                nextindex :221-236, simplify :243-311, LinearAlgorithm :397-502,
                                SearchLinearAlgorithm :604-673
  include/plinopt_library.inl   input2Temps :307-317, printmulorjustdiv :347-374, printSCA :376-386
  src/inplacer.cpp              FindProgram :38-80

Random draws (RANDOM_TIES) come from this build's per-candidate stream (include/plinopt_hip.h, CandRng): candidate `seed`
draws its row permutation (Fisher-Yates, the draws of the trilinear candidate without the sign bits), then the pivots of
variant 0 (unoriented, one draw per non-empty row), then the orientindex ties of variant 1 (oriented, appended).  The
unpermuted oriented program of :613 is the candidate BASE_SEED (no permutation draw), as `basec` of bin/trilplacer.
"""
from fractions import Fraction

BASE_SEED = (1 << 64) - 1
_M64 = (1 << 64) - 1


class CandRng:
    """include/plinopt_hip.h: splitmix64 of the seed -> GivRandom's LCG (x <- 950706376 x mod 2^31-1)."""

    def __init__(self, seed):
        x = (seed + 0x9E3779B97F4A7C15) & _M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
        x ^= x >> 31
        self.s = 1 + x % 2147483646

    def next(self):
        self.s = (950706376 * self.s) % 2147483647
        return self.s


# ----------------------------------------------------------------------------- Atom :15-124
class Atom:
    __slots__ = ("var", "src", "ope", "val", "des")

    def __init__(self, var, src, ope, val, des=-1):
        self.var, self.src, self.ope, self.val, self.des = var, src, ope, Fraction(val), des

    def copy(self):
        return Atom(self.var, self.src, self.ope, self.val, self.des)

    def sameops(self, p):                                          # :81-85
        return self.var == p.var and self.src == p.src and self.des == p.des

    def isnoop(self):                                              # :88-91
        return (addsub(self.ope) and self.val == 0) or (muldiv(self.ope) and self.val == 1)

    def cumulate(self, p):                                         # :94-122
        if self.sameops(p):
            if addsub(self.ope) and addsub(p.ope):
                self.val = self.val + p.val if self.ope == p.ope else self.val - p.val
                if self.val < 0:
                    self.ope = swapop(self.ope)
                    self.val = -self.val
                return True
            if muldiv(self.ope) and muldiv(p.ope):
                self.val = self.val * p.val if self.ope == p.ope else self.val / p.val
                if abs(self.val) < 1:
                    self.ope = invop(self.ope)
                    self.val = 1 / self.val
                return True
        return False

    def __str__(self):                                             # operator<< :37-77
        sca = muldiv(self.ope)
        if sca and self.val == 1:
            return ""
        if self.ope == " ":
            return "0;" if self.val == 0 else "%s%d;" % (self.var, self.src)
        out = "%s%d:=" % (self.var, self.src)
        uval = -self.val if self.val < 0 else self.val
        if sca:
            if self.val < 0:
                out += "-"
            out += print_sca(self.var, self.src, self.ope, uval)
        else:
            uope = swapop(self.ope) if self.val < 0 else self.ope
            out += "%s%d%s" % (self.var, self.src, uope) + printmulorjustdiv(self.var, self.des, uval)
        return out + ";"


def addsub(o):
    return o in "+-" and o != " "


def muldiv(o):
    return o in "*/" and o != " "


def swapop(o):
    return "-" if o == "+" else "+"


def invop(o):
    return "/" if o == "*" else "*"


def moneop(o, v):                                                  # MONEOP: the operation swapped when the pivot is -1
    return swapop(o) if v == -1 else o


def fstr(r):
    return str(r.numerator) if r.denominator == 1 else "%d/%d" % (r.numerator, r.denominator)


def printmulorjustdiv(c, i, r):                                    # plinopt_library.inl:360-374 (rationals)
    out = "%s%d" % (c, i)
    if r != 1:
        out += "/%d" % r.denominator if r.numerator == 1 else "*" + fstr(r)
    return out


def print_sca(c, i, p, r):                                         # plinopt_library.inl:376-386
    return printmulorjustdiv(c, i, r if p == "*" else 1 / r)


# ----------------------------------------------------------------------------- complexity :133-144
def complexity(prog):
    add = sca = rows = 0
    for a in prog:
        if addsub(a.ope):
            add += 1
            if a.val != 1 and a.val != -1:
                sca += 1
        if muldiv(a.ope):
            sca += 1
        if a.ope == " ":
            rows += 1
    return (add, sca, rows)


# ----------------------------------------------------------------------------- Pprint :163-175, input2Temps
def pprint(c, prog, P):
    """P[k] = the output row of the k-th barrier.  (The reference reads P[numop] for every barrier; this build maps the
    barriers of an appended program, k >= len(P), to P[k mod len(P)]: see DESIGN.md section 2.8.)"""
    lines, numop = [], 0
    for a in prog:
        head = ""
        if a.ope == " ":
            head = "%s%d:=" % (c, P[numop % len(P)])
            numop += 1
        lines.append(head + str(a))
    return "".join(s + "\n" for s in lines)


def input2temps(n, inv, tev):                                      # plinopt_library.inl:307-317
    return "".join("%s%d:=%s%d;\n" % (tev, i, inv, i) for i in range(n))


# ----------------------------------------------------------------------------- orientindex / nextindex :179-236
def orientindex(preci, L, rng):
    """L: the row as a list of (column, value), columns increasing.  Returns the index of the pivot in L."""
    nexti = next((k for k, (j, _) in enumerate(L) if j == preci), None)
    if nexti is None or L[nexti][1] != 1:
        vnext = [k for k, (_, v) in enumerate(L) if v == 1]
        if vnext:
            nexti = vnext[rng.next() % len(vnext)]                 # RANDOM_TIES: generator() % vnext.size()
    return nexti if nexti is not None else 0


def nextindex(preci, L, oriented, rng):
    if oriented:
        return orientindex(preci, L, rng)
    return rng.next() % len(L)                                     # std::shuffle(...).front(): one draw of the stream


# ----------------------------------------------------------------------------- simplify :243-311
def simplify(prog, transposed=False):
    n = len(prog)
    for i in range(n):
        it = prog[i]
        if it.ope == " ":
            continue
        for k in range(i + 1, len(prog)):
            nx = prog[k]
            if nx.sameops(it):
                c = it.copy()
                if c.cumulate(nx):
                    del prog[k]
                    if c.isnoop():
                        del prog[i]
                    else:
                        prog[i] = c
                    return True
            brk = it.src == nx.src and (nx.ope == " " or (addsub(it.ope) and muldiv(nx.ope)) or (muldiv(it.ope) and addsub(nx.ope)))
            if transposed:
                brk = brk or it.des == nx.src
            else:
                brk = brk or (it.des == nx.src and nx.ope != " ")
            brk = brk or it.src == nx.des
            if brk:
                break
    return False


# ----------------------------------------------------------------------------- LinearAlgorithm :397-502
def linear_algorithm(prog, rows, ncols, variable, oriented, rng):
    """Appends to `prog` (the reference's Program is never cleared here: :654 calls it on lProgram again).  transposed is
    false: FindProgram never sets it (src/inplacer.cpp:55-58, default of plinopt_inplace.h:44-45)."""
    preci = ncols
    for l, row in enumerate(rows):
        if row:
            ai = nextindex(preci, row, oriented, rng)
            i, av = row[ai]
            if av != 1:
                prog.append(Atom(variable, i, "*", av))                                   # :413-422
            for k, (j, v) in enumerate(row):
                if k != ai:
                    prog.append(Atom(variable, i, "+", v, j))                             # :431-434
            prog.append(Atom(variable, i, " ", av))                                       # :441
            for k, (j, v) in enumerate(row):
                if k != ai:
                    prog.append(Atom(variable, i, "-", v, j))                             # :451-454
            if av != 1:
                prog.append(Atom(variable, i, "/", av))                                   # :459-468
            if len(row) > 1:
                preci = i
        else:
            prog.append(Atom(" ", l, " ", 0))                                             # :474-476
    prog[:] = [a for a in prog if not (muldiv(a.ope) and a.val == 1)]                     # :480-481
    while simplify(prog, False):                                                          # :488-494
        pass
    return complexity(prog)


# ----------------------------------------------------------------------------- SearchLinearAlgorithm :604-673
def rows_of(m, n, ent):
    rows = [[] for _ in range(m)]
    for (i, j), v in sorted(ent.items()):
        rows[i].append((j, v))
    return rows


def transpose(m, n, ent):
    return n, m, {(j, i): v for (i, j), v in ent.items()}


def candidate(rows, ncols, seed):
    """One loop of :621-669 (or :613 for BASE_SEED).  Returns (perm, [(ops, program) of variant 0, of variant 1]); row l of
    the candidate's matrix is rows[perm[l]]."""
    m = len(rows)
    perm = list(range(m))
    rng = CandRng(seed)
    if seed == BASE_SEED:
        prog = []
        ops = linear_algorithm(prog, rows, ncols, "z", True, rng)
        return perm, [(ops, prog), (ops, prog)]
    for i in range(m, 1, -1):                                                             # :626-633 (Fisher-Yates)
        j = rng.next() % i
        perm[i - 1], perm[j] = perm[j], perm[i - 1]
    pa = [rows[r] for r in perm]
    lprog = []
    ops0 = linear_algorithm(lprog, pa, ncols, "z", False, rng)                           # :636
    prog0 = [a.copy() for a in lprog]
    ops1 = linear_algorithm(lprog, pa, ncols, "z", True, rng)                            # :654, lProgram not cleared
    return perm, [(ops0, prog0), (ops1, lprog)]


def cost6(rows, ncols, seed):
    _, v = candidate(rows, ncols, seed)
    return list(v[0][0]) + list(v[1][0])


def better(a, b):                                                                         # :637-641, :655-659
    return a[0] < b[0] or (a[0] == b[0] and a[1] < b[1])


def search(rows, ncols, seed0, nseeds):
    """The loop's best under (ADD, SCA, seed, variant), kept only when strictly better than the unpermuted oriented
    program.  Returns (ops, seed, variant) with seed = BASE_SEED when the incumbent stays."""
    inc = candidate(rows, ncols, BASE_SEED)[1][0][0]
    best = None
    for s in range(seed0, seed0 + nseeds):
        c = cost6(rows, ncols, s)
        for v in (0, 1):
            k = (c[3 * v], c[3 * v + 1], s, v)
            if best is None or k < best:
                best = k
                bops = tuple(c[3 * v:3 * v + 3])
    if best is not None and better(bops, inc):
        return bops, best[2], best[3]
    return inc, BASE_SEED, 0


def find_program(m, n, ent, transposed, seed0, nseeds):
    """FindProgram (src/inplacer.cpp:38-80): the stdout text and the counts."""
    inchar = "t" if transposed else "i"
    outdim = m if transposed else n
    if transposed:
        m, n, ent = transpose(m, n, ent)
    rows = rows_of(m, n, ent)
    ops, seed, var = search(rows, n, seed0, nseeds) if nseeds > 0 else (candidate(rows, n, BASE_SEED)[1][0][0], BASE_SEED, 0)
    perm, v = candidate(rows, n, seed)
    return input2temps(outdim, inchar, "z") + pprint("o", v[var][1], perm), ops
