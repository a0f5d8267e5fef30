"""Many-valued matrices with real CSE structure for the value-table modes of the HBM-resident kernel (plo_cse_big.hip: mode 1, value
table in LDS, 33 to 512 distinct coefficients; mode 0, in global memory, above 512), at moduli that are not Mersenne primes.  Pure
Python, fixed seeds, no input file.

Entry (i, j) = r_i * c_{b(i), j} mod p: r_i a row scaler, b(i) one of a few blocks.  The rows of a block share every column ratio, so
the pair triples (column, column, ratio) repeat and the CSE has work to do, while the number of distinct coefficients is about
(scalers) x (column values) and so can be set: tests/test_hbm_modes_cases_host.py pins both for every case, and
tests/test_gpu_hbm_modes.py runs the cases on the device against the literal oracle.

plan_info() restates the rules by which build_big_plan (plo_capi.hip) chooses a plan -- what plo_cse_plan_hbm_info reports -- from the
matrix and the modulus alone, so a device test can assert the path it claims to take."""
import random

P17 = 131071                                              # 2^17 - 1: the Mersenne control
P20, P21, P24, P25, P30 = 1048573, 2097143, 16777213, 33554393, 1073741789      # the largest primes below 2^20, 2^21, 2^24, 2^25, 2^30
INFO_FIELDS = ("mode", "idk", "defer", "wide", "rb", "kb", "bb", "NCmax", "nv", "agg_dual", "agg_cb", "mers", "invtab", "aggbits", "pbits", "hbits")
ENTRY_LIMIT = 1500                                        # the oracle's speed bounds the sizes


def _distinct(rng, k, p, avoid=()):
    out, seen = [], set(avoid)
    while len(out) < k:
        x = rng.randint(2, p - 2)
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def block_matrix(seed, p, m, n, nscal, ncolv, blocks=3, density=0.6, cols=None, contiguous=False, common=None, all_products=False, fresh=0, naive=None):
    """m x n, rows as {column: residue}.  Row i has the scaler r[i % nscal] and the block i % blocks (contiguous: i * blocks // m);
    the column values of a block come from a pool of ncolv residues, every one of them used; `cols` restricts the entries to
    those columns.
      common = (j0, j1, q): columns j0 < j1 are present in every row with entry(j1) / entry(j0) = q.
      all_products: every scaler meets every pool value somewhere, so the matrix has exactly nscal * ncolv distinct products.
      fresh: that many further entries with values that are no product.
      naive: entries are added (structured ones) or taken away until the rows' naive addition count, sum of (length - 1), is this."""
    rng = random.Random(seed)
    cols = list(range(n)) if cols is None else list(cols)
    scal = _distinct(rng, nscal, p)
    pool = _distinct(rng, ncolv, p, scal)
    slots = [(b, j) for b in range(blocks) for j in cols]
    rng.shuffle(slots)
    cval = {s: pool[k % ncolv] for k, s in enumerate(slots)}
    if common:
        j0, j1, q = common
        for b in range(blocks):
            cval[(b, j1)] = cval[(b, j0)] * q % p
    blk = (lambda i: i * blocks // m) if contiguous else (lambda i: i % blocks)
    ent = lambda i, j: scal[i % nscal] * cval[(blk(i), j)] % p
    rows = [{j: ent(i, j) for j in cols if rng.random() < density or (common and j in common[:2])} for i in range(m)]
    for i, r in enumerate(rows):
        if not r:
            r[cols[0]] = ent(i, cols[0])
    if all_products:
        have = {(i % nscal, cval[(blk(i), j)]) for i, r in enumerate(rows) for j in r}
        for s in range(nscal):
            for v in pool:
                if (s, v) not in have:
                    i, j = next((i, j) for i in range(s, m, nscal) for j in cols if cval[(blk(i), j)] == v)
                    rows[i][j] = ent(i, j)
    if naive is not None:
        cur = sum(len(r) - 1 for r in rows)
        order = [(i, j) for i in range(m) for j in cols]
        rng.shuffle(order)
        for i, j in order:
            if cur < naive and j not in rows[i]:
                rows[i][j] = ent(i, j)
                cur += 1
            elif cur > naive and j in rows[i] and len(rows[i]) > 2 and not all_products and not (common and j in common[:2]):
                del rows[i][j]
                cur -= 1
        assert cur == naive
    used = {x for r in rows for x in r.values()}
    for w in _distinct(rng, fresh, p, used):
        i, j = next((i, j) for i in range(m) for j in cols if j not in rows[i])
        rows[i][j] = w
    return rows


def one_more_entry(rows, p):
    """the same matrix with one more entry (a value the matrix already has) in the first row that has room"""
    rows = [dict(r) for r in rows]
    n = 1 + max(j for r in rows for j in r)
    i, j = next((i, j) for i, r in enumerate(rows) for j in range(n) if j not in r)
    rows[i][j] = rows[i][min(rows[i])]
    return rows


def to_csr(rows, p):
    rp, c, v = [0], [], []
    for r in rows:
        for j, x in sorted(r.items()):
            assert 0 < x < p
            c.append(j)
            v.append(x)
        rp.append(len(c))
    return rp, c, v


def naive_additions(rows):
    return sum(len(r) - 1 for r in rows)


def triples(rows, p):
    """{(first column, second column, ratio second / first): frequency}: the pair triples of the input"""
    T = {}
    for r in rows:
        e = sorted(r.items())
        inv = [pow(x, p - 2, p) for _, x in e]
        for x in range(len(e)):
            for y in range(x + 1, len(e)):
                k = (e[x][0], e[y][0], e[y][1] * inv[x] % p)
                T[k] = T.get(k, 0) + 1
    return T


def _clog2(x):
    l = 0
    while (1 << l) < x:
        l += 1
    return l


class Refused(Exception):
    """the plan rules answer PLO_E_CAPACITY with this text"""


def plan_info(m, n, rows, p, eager=False, wide=False):
    """The 16 words of plo_cse_plan_hbm_info as build_big_plan's rules give them (no knob but PLO_BIG_EAGER and PLO_BIG_WIDE)."""
    lens = [len(r) for r in rows]
    nnz, naive = sum(lens), sum(l - 1 for l in lens if l > 1)
    vals = sorted({x for r in rows for x in r.values()})
    nv = len(vals)
    ratio_ids = nv <= 32
    rb = _clog2(p)
    NC = n + naive // 2 + 2
    # the ratio field of a 48-bit pair key: the residue while that leaves room for the columns, else the ratio's identifier (<= 32 values only)
    bbres = (48 - rb) // 2 if rb <= 44 else 0
    fits = rb <= 30 and bbres >= 2 and n + 2 <= (1 << bbres) and min(NC, 32768) <= (1 << bbres)
    kb, idk = rb, 0
    if not fits and ratio_ids and rb <= 31:
        inv = {v: pow(v, p - 2, p) for v in vals}
        nr = len({a * inv[b] % p for a in vals for b in vals})
        idk, kb = 1, max(1, _clog2(nr))
    elif rb > 30 or bbres < 2 or (bbres < 15 and not fits):
        raise Refused("modulus too large for the 48-bit pair key")
    bbmax = min(15, (48 - kb) // 2)
    if n + 2 > (1 << bbmax) or n + 2 > 32768:
        raise Refused("too many columns")
    NC = min(NC, 1 << bbmax, 32768)
    bb = _clog2(NC)
    T = triples(rows, p)
    pairs0 = sum(T.values())
    if idk:
        rv = sorted({a * inv[b] % p for a in vals for b in vals})
        rid = {x: k for k, x in enumerate(rv)}
    key = lambda a, b, q: (a << (bb + kb)) | (b << kb) | (rid[q] if idk else q)
    keys = sorted(key(*t) for t, f in T.items() if f >= 2)             # triples of frequency 1 are pruned
    maxf = max(T.values()) if T else 0
    multcap = min(naive // 2 + 8, NC)
    cap = 1024
    while cap < 2 * len(keys) + 1024 or cap < 2 * nnz + 2 * multcap + 64:
        cap <<= 1
    hbits = _clog2(cap)
    # deferred updates: taken when a partition of the store and its share of the log fit the merge's LDS table
    defer, pbits = 0, 0
    if not eager:
        topsum = sum(sorted(lens, reverse=True)[:maxf])
        pb = 0
        while (len(keys) >> pb) > 1280 and pb < 11:
            pb += 1
        fill = [0] * (1 << pb)
        for k in keys:
            fill[((k * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF) >> (64 - pb) if pb else 0] += 1
        maxfill = max(fill)
        capp = (maxfill + maxfill // 4 + 64 + 1) & ~1
        hotmax = min(1 << 17, pairs0)
        stepmax = 3 * topsum + 3 * 8192
        if capp <= 5000 and (6080 - capp) * (1 << pb) * 5 // 6 > stepmax + hotmax + 4096:
            defer, pbits = 1, pb
            pg = 1024
            while pg < 2 * nnz + 2 * multcap + 64:
                pg <<= 1
            hbits = _clog2(pg)
    aggbits = min(13, max(6, _clog2(min(4 * pairs0 + 64, 1 << 13))))
    # an LDS aggregation entry carries the ratio and its inverse when both fit beside the column and a count up to m
    cb = _clog2(m + 2)
    if bb + 2 * rb + cb <= 64:
        agg_dual, agg_cb = 1, min(16, 64 - bb - 2 * rb)
    else:
        agg_dual, agg_cb = 0, 16
    mers = next((k for k in range(2, 31) if p == (1 << k) - 1), 0)
    mode = 2 if ratio_ids else 1 if nv <= 512 else 0
    return dict(mode=mode, idk=idk, defer=defer, wide=1 if wide else 0, rb=rb, kb=kb, bb=bb, NCmax=NC, nv=nv, agg_dual=agg_dual, agg_cb=agg_cb,
                mers=mers, invtab=1 if p <= (1 << 20) else 0, aggbits=aggbits, pbits=pbits, hbits=hbits)


class Case:
    """One matrix at one modulus.  `info`: the fields of the plan (default plan) this case is in the suite for; `nv`, the exact number of distinct
    coefficients; `floor`, how far below the naive count the oracle's additions must lie on every seed the device test uses."""
    def __init__(self, name, p, m, n, seed0, gen, nv, info, floor=200, refused=None, knob=None):
        self.name, self.p, self.m, self.n, self.seed0, self.gen, self.nv, self.info, self.floor, self.refused, self.knob = name, p, m, n, seed0, gen, nv, info, floor, refused, knob
        self._rows = None

    @property
    def rows(self):
        if self._rows is None:
            self._rows = self.gen(self.p)
        return self._rows

    def csr(self):
        return to_csr(self.rows, self.p)

    def plan_info(self, eager=False):
        return plan_info(self.m, self.n, self.rows, self.p, eager=eager, wide=self.knob == "PLO_BIG_WIDE")

    def __repr__(self):
        return self.name


NSEEDS = 6
LDS = dict(nscal=6, ncolv=8)                    # 46 products in use: mode 1
GLB = dict(nscal=60, ncolv=24)                  # above 512: mode 0
FAR = [0, 1, 2, 3] + list(range(270, 290))      # group (d): the frequent triples start at a column of 256 and more


def _a(kw, seed):
    return lambda p: block_matrix(seed, p, 60, 24, density=0.58, **kw)


def _b(kw):
    return lambda p: block_matrix(21, p, 64, 24, all_products=True, density=0.5, **kw)


def _c(m):
    return lambda p: block_matrix(31, p, m, 12, nscal=6, ncolv=8, common=(0, 1, 3))


def _d(p):
    return block_matrix(41, p, 30, 300, nscal=30, ncolv=24, cols=FAR)


def _g512(p):
    return block_matrix(51, p, 60, 24, naive=973, density=0.7, **LDS)


def _h(kw):
    return lambda p: block_matrix(61, p, 30, 48, blocks=10, density=1.0, contiguous=True, **kw)


def _cases():
    C = []
    s0 = iter(range(1000, 100000, 1000))
    add = lambda *a, **k: C.append(Case(a[0], a[1], a[2], a[3], next(s0), *a[4:], **k))
    # (a) both modes at the five primes and at the Mersenne control: the same two matrix shapes throughout.  (The residues are drawn below
    # the modulus, so the number of values of the second shape moves with it.)
    agg = {P17: (1, 16), P20: (1, 15), P21: (1, 13), P24: (1, 7), P25: (0, 16), P30: (0, 16)}
    for p in (P17, P20, P21, P24, P25, P30):
        for tag, kw, seed, mode, nv in (("lds", LDS, 11, 1, 46), ("global", GLB, 12, 0, 671 if p == P17 else 673)):
            add("a-%s-%d" % (tag, p), p, 60, 24, _a(kw, seed), nv,
                dict(mode=mode, idk=0, mers=17 if p == P17 else 0, invtab=1 if p <= P20 else 0, agg_dual=agg[p][0], agg_cb=agg[p][1], bb=9, kb=_clog2(p)))
    # (b) value-count boundaries: 32 | 33 (mode 2 | 1) and 512 | 513 (mode 1 | 0): all products of scalers and column values, plus one fresh value
    for nv, p, mode, kw in ((32, P21, 2, dict(nscal=4, ncolv=8)), (33, P21, 1, dict(nscal=4, ncolv=8, fresh=1)),
                            (512, P25, 1, dict(nscal=16, ncolv=32)), (513, P25, 0, dict(nscal=16, ncolv=32, fresh=1))):
        add("b-%d-values" % nv, p, 64, 24, _b(kw), nv, dict(mode=mode, idk=0, mers=0, invtab=0, nv=nv))
    # (c) the agg_dual boundary at 2^24: 9 column bits + 2 x 24 ratio bits leave 7 for a count up to m + 1: 126 rows fit, 127 do not.
    # The triple (0, 1, 3) is in every row: a count of m in the entry.
    for m, dual, cb in ((126, 1, 7), (127, 0, 16)):
        add("c-%d-rows" % m, P24, m, 12, _c(m), 48, dict(mode=1, idk=0, mers=0, invtab=0, bb=9, agg_dual=dual, agg_cb=cb), floor=100)
    # (d) bit 47 of a key (bit 63 of a table, store or log record): 9 column bits beside a 30-bit residue, first columns of 256 and more
    for p, dual, cb in ((P30, 0, 16), (P25, 1, 5)):
        add("d-far-columns-%d" % p, p, 30, 300, _d, 362, dict(mode=1, idk=0, mers=0, invtab=0, bb=9, kb=_clog2(p), NCmax=502, agg_dual=dual, agg_cb=cb))
    # (f) the kernels with 64-bit workspace offsets, one case of (a) per mode
    for tag, kw, seed, mode, nv in (("lds", LDS, 11, 1, 46), ("global", GLB, 12, 0, 673)):
        add("f-wide-%s" % tag, P21, 60, 24, _a(kw, seed), nv, dict(mode=mode, wide=1, mers=0, invtab=0, agg_dual=1, agg_cb=13), knob="PLO_BIG_WIDE")
    # (g) the refusal boundary at 2^30, 9 column bits: a column bound of 512 is taken, 513 is refused -- unless the matrix has at most 32
    # values, whose keys then hold ratio identifiers
    add("g-512-columns", P30, 60, 24, _g512, 48, dict(mode=1, idk=0, bb=9, kb=30, NCmax=512, agg_dual=0))
    add("g-513-columns", P30, 60, 24, lambda p: one_more_entry(_g512(p), p), 48, None, refused="48-bit pair key")
    add("g-513-columns-32-values", P30, 60, 24, lambda p: block_matrix(52, p, 60, 24, naive=974, density=0.7, nscal=4, ncolv=8), 32, dict(mode=2, idk=1, bb=10, NCmax=513))
    # (h) deferred updates (hot table, partitioned store and log instead of the one pair table) need more than 10240 distinct triples of
    # frequency 2 and more: 30 rows in 10 blocks of 3 over 48 full columns have 11280
    for tag, p, kw, mode, nv, dual, cb in (("lds", P25, dict(nscal=3, ncolv=40), 1, 120, 0, 16), ("lds", P21, dict(nscal=3, ncolv=40), 1, 120, 1, 12),
                                           ("global", P25, dict(nscal=15, ncolv=48), 0, 642, 0, 16)):
        add("h-deferred-%s-%d" % (tag, p), p, 30, 48, _h(kw), nv, dict(mode=mode, idk=0, defer=1, pbits=4, mers=0, invtab=0, agg_dual=dual, agg_cb=cb, bb=10))
    return C


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
ARGMIN = ("a-lds-%d" % P25, "a-global-%d" % P21)      # (e): plan.search under the three cost orders, one case per mode
ARGMIN_SEEDS = 64

_oracle_costs = {}


def oracle_costs(case):
    """(adds[], muls[]) of the literal oracle on the case's NSEEDS seeds: computed once, shared by the tests"""
    if case.name not in _oracle_costs:
        from plo_testlib import OracleMatrix
        rp, c, v = case.csr()
        _oracle_costs[case.name] = tuple(OracleMatrix(case.m, case.n, rp, c, v, case.p).cost_many(seed0=case.seed0, nseeds=NSEEDS, nthreads=NSEEDS))
    return _oracle_costs[case.name]
