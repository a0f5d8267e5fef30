"""Host-side mirror of the reference's restart-loop interface for the CSE path.

`CSEOptimiser(nbops, sout, F, M, T, global, randomloops, verbose)`
(reference include/plinopt_optimize.inl:1193-1247) runs `randomloops`
independent candidates and keeps the best (adds, muls) under `cmpOpCount`
(include/plinopt_optimize.h:53-64).  Here the loop body runs on the GPU through
libplinopt_hip.so; this module only marshals arguments.
"""
import ctypes

from . import capi


class CSEPlan:
    """A matrix over Z_p prepared once and resident in HBM (plo_cse_plan_create)."""

    def __init__(self, m, n, rowptr, col, val, p, device=None, hbm=False):
        L = capi.lib()
        if device is not None:
            capi.check(L.plo_init(int(device)))
        self.m, self.n, self.p = m, n, p
        self.nnz = len(col)
        csr, self._keep = capi.make_csr(m, n, rowptr, col, val)
        h = ctypes.c_void_p()
        capi.check(L.plo_cse_plan_create_ex(ctypes.byref(csr), p, capi.PLAN_HBM if hbm else 0, ctypes.byref(h)))
        self._h = h
        self.is_hbm = bool(L.plo_cse_plan_is_hbm(h))     # HBM-resident kernel family (one workgroup per candidate)
        self.last_stats = None

    def close(self):
        if getattr(self, "_h", None):
            capi.lib().plo_cse_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hbm_counters(self):
        """Diagnostics of the HBM-resident family over the last launch (plo_cse_plan_hbm_counters)."""
        out = (ctypes.c_uint32 * 13)()
        capi.check(capi.lib().plo_cse_plan_hbm_counters_ex(self._h, out, 13))
        return dict(zip(("steps", "full_scans", "level_rebuilds", "bisections", "spilled_pairs", "list_overflows", "candidates", "eager_refits", "extra_sweep_windows", "rows_searched",
                         "forced_merges", "merge_groups", "merge_loop_records"), out[:13]))

    HBM_INFO = ("mode", "idk", "defer", "wide", "rb", "kb", "bb", "NCmax", "nv", "agg_dual", "agg_cb", "mers", "invtab", "aggbits", "pbits", "hbits")

    def hbm_info(self):
        """What the plan of the HBM-resident family chose (plo_cse_plan_hbm_info: host only, nothing is launched)."""
        out = (ctypes.c_uint32 * 16)()
        capi.check(capi.lib().plo_cse_plan_hbm_info(self._h, out))
        return dict(zip(self.HBM_INFO, out[:16]))

    def cost_many(self, seeds=None, seed0=0, n=0):
        """(adds[], muls[]) of candidates `seeds` (or seed0..seed0+n-1): Optimizer() per seed."""
        L = capi.lib()
        if seeds is not None:
            n = len(seeds)
            sp = (ctypes.c_uint64 * max(n, 1))(*seeds)
        else:
            sp = None
        adds = (ctypes.c_uint32 * max(n, 1))()
        muls = (ctypes.c_uint32 * max(n, 1))()
        st = capi.Stats()
        capi.check(L.plo_cse_cost_many_plan(self._h, sp, seed0, n, adds, muls, ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return list(adds[:n]), list(muls[:n])

    def search(self, seed0, nseeds, cost_mode=capi.COST_SUM_THEN_ADD):
        """Best (adds, muls, seed) over seeds seed0..seed0+nseeds-1, ties to the smallest seed."""
        L = capi.lib()
        b, st = capi.Best(), capi.Stats()
        capi.check(L.plo_cse_search_plan(self._h, seed0, nseeds, cost_mode, ctypes.byref(b), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return b.adds, b.muls, b.seed

    # -E: RecSub's schedule tree walked by index (include/plinopt_hip.h)
    def enum_cost_many(self, first, n):
        """(adds, muls, product of radices) of the schedules first..first+n-1"""
        L = capi.lib()
        adds = (ctypes.c_uint32 * max(n, 1))(); muls = (ctypes.c_uint32 * max(n, 1))(); prods = (ctypes.c_uint64 * max(n, 1))()
        st = capi.Stats()
        capi.check(L.plo_cse_enum_cost_many_plan(self._h, first, n, adds, muls, prods, ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return list(adds[:n]), list(muls[:n]), list(prods[:n])

    def enum_search(self, first, count, cost_mode=capi.COST_ADD_THEN_MUL):
        """Best (adds, muls, index) over the schedules first..first+count-1 and the largest radix product seen: the
        enumeration from 0 is exhaustive once count >= that product."""
        L = capi.lib()
        b, st, mp = capi.Best(), capi.Stats(), ctypes.c_uint64()
        capi.check(L.plo_cse_enum_search_plan(self._h, first, count, cost_mode, ctypes.byref(b), ctypes.byref(mp), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return (b.adds, b.muls, b.seed), mp.value


def cse_q_universe(m, n, rowptr, col, num, den=None):
    """Host only (plo_cse_q_universe): (prime, |V|, U) of a rational matrix, U ascending over Q as (num, den) pairs -- every value a
    candidate of the exact search over Q can compare, and the prime that keeps their residues apart."""
    L = capi.lib()
    A, keep = _qcsr(m, n, rowptr, col, num, den)
    prime, nv, nu = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    rc = L.plo_cse_q_universe(ctypes.byref(A), ctypes.byref(prime), ctypes.byref(nv), ctypes.byref(nu), None, None, 0)
    if rc != capi.PLO_E_CAPACITY or nu.value == 0:
        capi.check(rc)
    un, ud = (ctypes.c_int64 * nu.value)(), (ctypes.c_int64 * nu.value)()
    capi.check(L.plo_cse_q_universe(ctypes.byref(A), ctypes.byref(prime), ctypes.byref(nv), ctypes.byref(nu), un, ud, nu.value))
    del keep
    return prime.value, nv.value, list(zip(un, ud))


class CSEPlanQ(CSEPlan):
    """A matrix over the RATIONALS prepared for the restart search that is bit-exact with Optimizer() over Q
    (plo_cse_plan_create_q): entries num[k]/den[k] (den None: integers).  cost_many and search are CSEPlan's; the schedule
    enumeration is refused on such a plan."""

    def __init__(self, m, n, rowptr, col, num, den=None, device=None):
        L = capi.lib()
        if device is not None:
            capi.check(L.plo_init(int(device)))
        self.m, self.n, self.p = m, n, 0
        self.nnz = len(col)
        A, self._keep = _qcsr(m, n, rowptr, col, num, den)
        h = ctypes.c_void_p()
        capi.check(L.plo_cse_plan_create_q(ctypes.byref(A), 0, ctypes.byref(h)))
        self._h = h
        self.is_hbm = False
        self.last_stats = None
        self.prime = cse_q_universe(m, n, rowptr, col, num, den)[0]      # the prime the plan took (the same host code chooses it)


def cse_search_multi(m, n, rowptr, col, val, p, seed0, nseeds, devices, cost_mode=capi.COST_SUM_THEN_ADD):
    """One process, several devices (plo_cse_search_multi): the restart range in len(devices) contiguous shards, one host thread and
    one device each; (adds, muls, seed) of the minimum under (cmpOpCount key, seed) and the aggregated stats."""
    L = capi.lib()
    csr, keep = capi.make_csr(m, n, rowptr, col, val)
    devs = (ctypes.c_int * len(devices))(*devices)
    b, st = capi.Best(), capi.Stats()
    capi.check(L.plo_cse_search_multi(ctypes.byref(csr), p, seed0, nseeds, cost_mode, len(devices), devs, ctypes.byref(b), ctypes.byref(st)))
    del keep
    return (b.adds, b.muls, b.seed), {"seconds": st.seconds, "kernel_ms": st.kernel_ms, "candidates": st.candidates, "launches": st.launches, "reduce": st.reduce}


def cmp_op_count_key(adds, muls, cost_mode=capi.COST_SUM_THEN_ADD):
    """Sort key equivalent to cmpOpCount (include/plinopt_optimize.h:53-64)."""
    if cost_mode == capi.COST_ADD_THEN_MUL:
        return (adds, muls)
    if cost_mode == capi.COST_SUM:
        return (adds + muls,)
    return (adds + muls, adds)


class CSEChain:
    """Two matrices per candidate with one random stream: the restart loop of `LUOptimiser`
    (reference include/plinopt_optimize.inl:1056-1100) -- Optimizer() on U, then on L, costs added."""

    def __init__(self, first, second, p, device=None):
        L = capi.lib()
        if device is not None:
            capi.check(L.plo_init(int(device)))
        c1, self._k1 = capi.make_csr(*first)
        c2, self._k2 = capi.make_csr(*second)
        h = ctypes.c_void_p()
        capi.check(L.plo_cse_chain_create(ctypes.byref(c1), ctypes.byref(c2), p, ctypes.byref(h)))
        self._h = h
        self.last_stats = None

    def close(self):
        if getattr(self, "_h", None):
            capi.lib().plo_cse_chain_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def cost_many(self, seeds=None, seed0=0, n=0):
        L = capi.lib()
        if seeds is not None:
            n = len(seeds)
            sp = (ctypes.c_uint64 * max(n, 1))(*seeds)
        else:
            sp = None
        adds = (ctypes.c_uint32 * max(n, 1))()
        muls = (ctypes.c_uint32 * max(n, 1))()
        st = capi.Stats()
        capi.check(L.plo_cse_chain_cost_many(self._h, sp, seed0, n, adds, muls, ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return list(adds[:n]), list(muls[:n])

    def search(self, seed0, nseeds, cost_mode=capi.COST_SUM_THEN_ADD):
        L = capi.lib()
        b, st = capi.Best(), capi.Stats()
        capi.check(L.plo_cse_chain_search(self._h, seed0, nseeds, cost_mode, ctypes.byref(b), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return b.adds, b.muls, b.seed


def chain_batch(pairs, p, seed0, per_pair, cost_mode=capi.COST_SUM_THEN_ADD, want_costs=True):
    """Many chained pairs in one launch (`plo_cse_chain_batch`): pairs = [((m,n,rowptr,col,val), (m,n,rowptr,col,val)), ...];
    candidate c runs on pair c // per_pair with seed seed0 + c.  Returns (adds, muls, (best adds, best muls, best seed), stats)."""
    L = capi.lib()
    keep, firsts, seconds = [], (capi.CSR * len(pairs))(), (capi.CSR * len(pairs))()
    for k, (A, B) in enumerate(pairs):
        for dst, (m, n, rp, col, val) in ((firsts, A), (seconds, B)):
            a = ((ctypes.c_uint32 * len(rp))(*rp), (ctypes.c_uint32 * max(len(col), 1))(*col), (ctypes.c_uint32 * max(len(val), 1))(*val))
            keep.append(a)
            dst[k] = capi.CSR(m, n, a[0], a[1], a[2])
    n = len(pairs) * per_pair
    adds = (ctypes.c_uint32 * n)() if want_costs else None
    muls = (ctypes.c_uint32 * n)() if want_costs else None
    b, st = capi.Best(), capi.Stats()
    capi.check(L.plo_cse_chain_batch(len(pairs), firsts, seconds, p, seed0, per_pair, cost_mode, adds, muls, ctypes.byref(b), ctypes.byref(st)))
    return (list(adds) if want_costs else None), (list(muls) if want_costs else None), (b.adds, b.muls, b.seed), st.as_dict()


def cse_batch_search(firsts, seconds, p, seed0, per_problem, cost_mode=capi.COST_SUM_THEN_ADD):
    """Many independent restart searches in one call (`plo_cse_batch_search`): firsts = [(m,n,rowptr,col,val), ...], seconds the
    same for the chained search of pairs, or None; candidate j of problem q has seed seed0 + q*per_problem + j.  Returns
    ([(best adds, best muls, best seed) per problem], [status per problem], stats); a problem the wave kernel refuses has its
    code in status and (2^32-1, 2^32-1, 2^64-1) as best."""
    L = capi.lib()
    nprob = len(firsts)
    if seconds is not None and len(seconds) != nprob:
        raise ValueError("firsts and seconds differ in length")
    keep = []

    def array(mats):
        arr = (capi.CSR * max(len(mats), 1))()
        for k, (m, n, rp, col, val) in enumerate(mats):
            a = ((ctypes.c_uint32 * len(rp))(*rp), (ctypes.c_uint32 * max(len(col), 1))(*col), (ctypes.c_uint32 * max(len(val), 1))(*val))
            keep.append(a)
            arr[k] = capi.CSR(m, n, a[0], a[1], a[2])
        return arr
    A = array(firsts)
    B = array(seconds) if seconds is not None else None
    bests, status, st = (capi.Best * max(nprob, 1))(), (ctypes.c_int32 * max(nprob, 1))(), capi.Stats()
    capi.check(L.plo_cse_batch_search(nprob, A, B, p, seed0, per_problem, cost_mode, bests, status, ctypes.byref(st)))
    return [(b.adds, b.muls, b.seed) for b in bests[:nprob]], list(status[:nprob]), st.as_dict()


def kernel_search(M, p, seed0, nrestarts, per_block=1, cost_mode=capi.COST_SUM_THEN_ADD, want_costs=True):
    """The kernel method with decomposition, images and both Optimizer calls on the device (`plo_kernel_search`):
    M = (m, n, rowptr, col, val).  Returns (adds, muls, info, (best adds, best muls, best seed), stats); info[c] =
    (rank, NotIndep, dependent rows) of restart c."""
    L = capi.lib()
    m, n, rp, col, val = M
    A, keep = capi.make_csr(m, n, rp, col, val)
    adds = (ctypes.c_uint32 * nrestarts)() if want_costs else None
    muls = (ctypes.c_uint32 * nrestarts)() if want_costs else None
    info = (ctypes.c_uint32 * (3 * nrestarts))() if want_costs else None
    b, st = capi.Best(), capi.Stats()
    capi.check(L.plo_kernel_search(ctypes.byref(A), p, seed0, nrestarts, per_block, cost_mode, adds, muls, info, ctypes.byref(b), ctypes.byref(st)))
    del keep
    inf = [tuple(info[3 * k:3 * k + 3]) for k in range(nrestarts)] if want_costs else None
    return (list(adds) if want_costs else None), (list(muls) if want_costs else None), inf, (b.adds, b.muls, b.seed), st.as_dict()


def kernel_search_orders(M, p, seed0, first, count, sub=1, cost_mode=capi.COST_SUM_THEN_ADD, want_costs=True):
    """The kernel method over prescribed row orders (`plo_kernel_search_orders`, `bin/optimizer -N`): candidate c is restart
    c % sub of the (first + c // sub)-th permutation of the rows in lexicographic order.  M = (m, n, rowptr, col, val).  Returns
    (adds, muls, info, (best adds, best muls, best seed), stats); the winner's order index is (best seed - seed0) // sub."""
    L = capi.lib()
    m, n, rp, col, val = M
    A, keep = capi.make_csr(m, n, rp, col, val)
    nc = count * sub
    adds = (ctypes.c_uint32 * max(nc, 1))() if want_costs else None
    muls = (ctypes.c_uint32 * max(nc, 1))() if want_costs else None
    info = (ctypes.c_uint32 * max(3 * nc, 1))() if want_costs else None
    b, st = capi.Best(), capi.Stats()
    capi.check(L.plo_kernel_search_orders(ctypes.byref(A), p, seed0, first, count, sub, cost_mode, adds, muls, info, ctypes.byref(b), ctypes.byref(st)))
    del keep
    inf = [tuple(info[3 * k:3 * k + 3]) for k in range(nc)] if want_costs else None
    return (list(adds[:nc]) if want_costs else None), (list(muls[:nc]) if want_costs else None), inf, (b.adds, b.muls, b.seed), st.as_dict()


def kernel_batch_search(mats, p, seed0, per_problem, cost_mode=capi.COST_SUM_THEN_ADD):
    """The kernel method on many matrices in one call (`plo_kernel_batch_search`): mats = [(m,n,rowptr,col,val), ...]; restart j of
    problem q has seed seed0 + q*per_problem + j, for its decomposition too (`kernel_search(..., per_block=1)`).  Returns
    ([(best adds, best muls, best seed) per problem], [status per problem], stats); a problem the device code refuses has its
    code in status and (2^32-1, 2^32-1, 2^64-1) as best."""
    L = capi.lib()
    nprob = len(mats)
    keep, arr = [], (capi.CSR * max(nprob, 1))()
    for k, (m, n, rp, col, val) in enumerate(mats):
        a = ((ctypes.c_uint32 * len(rp))(*rp), (ctypes.c_uint32 * max(len(col), 1))(*col), (ctypes.c_uint32 * max(len(val), 1))(*val))
        keep.append(a)
        arr[k] = capi.CSR(m, n, a[0], a[1], a[2])
    bests, status, st = (capi.Best * max(nprob, 1))(), (ctypes.c_int32 * max(nprob, 1))(), capi.Stats()
    capi.check(L.plo_kernel_batch_search(nprob, arr, p, seed0, per_problem, cost_mode, bests, status, ctypes.byref(st)))
    del keep
    return [(b.adds, b.muls, b.seed) for b in bests[:nprob]], list(status[:nprob]), st.as_dict()


def kernel_search_multi(M, p, seed0, nrestarts, devices, cost_mode=capi.COST_SUM_THEN_ADD):
    """`plo_kernel_search_multi`: the restart loop of the kernel method over the listed devices from this process (one host thread
    and one device per contiguous shard, minimum by the RCCL MIN all-reduces).  Returns ((adds, muls, seed), stats)."""
    L = capi.lib()
    m, n, rp, col, val = M
    A, keep = capi.make_csr(m, n, rp, col, val)
    dv = (ctypes.c_int * len(devices))(*devices)
    b, st = capi.Best(), capi.Stats()
    capi.check(L.plo_kernel_search_multi(ctypes.byref(A), p, seed0, nrestarts, 1, cost_mode, len(devices), dv, ctypes.byref(b), ctypes.byref(st)))
    del keep
    return (b.adds, b.muls, b.seed), st.as_dict()


def tril_search_multi(m, mats, seed0, nseeds, devices, expanded=False):
    """`plo_tril_search_multi` (BASELINE configs[3]): the restart loop of SearchTriLinearAlgorithm over the listed devices from this
    process.  mats = three (n, rowptr, col, num[, den]) triples as for TrilPlan.  Returns (((ADD, SCA, MUL), seed, variant), stats)."""
    L = capi.lib()
    keep, cs = [], []
    for t in mats:
        n, rowptr, col, val = t[:4]
        den = t[4] if len(t) == 5 else [1] * len(val)
        a = ((ctypes.c_uint32 * len(rowptr))(*rowptr), (ctypes.c_uint32 * max(len(col), 1))(*col), (ctypes.c_int64 * max(len(val), 1))(*[int(x) for x in val]),
             (ctypes.c_int64 * max(len(den), 1))(*[int(x) for x in den]))
        keep.append(a)
        cs.append(capi.QCSR(m, n, a[0], a[1], a[2], a[3]))
    dv = (ctypes.c_int * len(devices))(*devices)
    b, st = capi.TrilBest(), capi.Stats()
    capi.check(L.plo_tril_search_multi(ctypes.byref(cs[0]), ctypes.byref(cs[1]), ctypes.byref(cs[2]), int(bool(expanded)), seed0, nseeds, len(devices), dv,
                                       ctypes.byref(b), ctypes.byref(st)))
    del keep
    return ((b.add, b.sca, b.mul), b.seed, b.variant), st.as_dict()


def cob_search(n, m, TM, Cand, row, offsetblock, coeffs, p, w0=-1, w1=-1, groups=None):
    """One (block,row) enumeration of `localSparsifier` (reference include/plinopt_sparsify.inl:282-314) on the
    GPU: |coeffs|^4 candidate rows through `testLinComb`.  TM (n x m) and Cand (n x n) are flat row-major lists of
    residues.  groups = (first, count): only the (i,j,k) prefixes first..first+count-1 (a shard, plo_cob_search_range).
    Returns ((zeros_v, zeros_w, index, found), stats)."""
    L = capi.lib()
    b, st = capi.CobBest(), capi.Stats()
    arr = lambda xs: (ctypes.c_uint32 * max(len(xs), 1))(*xs)
    g0, gn = groups if groups is not None else (0, len(coeffs) ** 3)
    capi.check(L.plo_cob_search_range(n, m, arr(TM), arr(Cand), row, offsetblock, arr(coeffs), len(coeffs), p, w0, w1, g0, gn,
                                      ctypes.byref(b), ctypes.byref(st)))
    return (b.zeros_v, b.zeros_w, b.index, b.found), st.as_dict()


def cob_search_batch(n, m, row, offsetblock, problems):
    """Up to 4 enumerations of the same shape in ONE launch (`plo_cob_search_batch`): problems = [(TM, Cand, coeffs, p, w0, w1), ...]
    (the two primes of an enumeration over the rationals).  Returns ([(zeros_v, zeros_w, index, found), ...], stats)."""
    L = capi.lib()
    arr = lambda xs: (ctypes.c_uint32 * max(len(xs), 1))(*xs)
    keep, pr = [], (capi.CobProblem * len(problems))()
    for k, (TM, Cand, coeffs, p, w0, w1) in enumerate(problems):
        a, b, c = arr(TM), arr(Cand), arr(coeffs); keep += [a, b, c]
        pr[k] = capi.CobProblem(ctypes.cast(a, ctypes.POINTER(ctypes.c_uint32)), ctypes.cast(b, ctypes.POINTER(ctypes.c_uint32)),
                                ctypes.cast(c, ctypes.POINTER(ctypes.c_uint32)), len(coeffs), p, w0, w1)
    out, st = (capi.CobBest * len(problems))(), capi.Stats()
    capi.check(L.plo_cob_search_batch(len(problems), n, m, row, offsetblock, pr, out, ctypes.byref(st)))
    return [(b.zeros_v, b.zeros_w, b.index, b.found) for b in out], st.as_dict()


TRIL_BASE_SEED = (1 << 64) - 1


class TrilPlan:
    """Mirror of the restart loop of `SearchTriLinearAlgorithm` (reference include/plinopt_inplace.inl:812-929):
    A, B and T (= transpose of the product matrix) as integer CSR triples (rowptr, col, val) with m rows each.
    `cost_many` returns, per seed, ((ADD,SCA,MUL) oriented, (ADD,SCA,MUL) unoriented); `search` the best
    (ADD, SCA, MUL, seed, variant) under the reference's order (:893-897), ties to the smaller (seed, variant)."""

    def __init__(self, m, mats, device=None, expanded=False):
        """expanded: `trilplacer -e` (TransposedDoubleAlgorithm on the double expansion of T)"""
        L = capi.lib()
        if device is not None:
            capi.check(L.plo_init(device))
        self._keep = []
        cs = []
        rational = any(len(t) == 5 for t in mats)            # (n, rowptr, col, num, den): rational coefficients (plo_tril_plan_create_q)
        for t in mats:
            n, rowptr, col, val = t[:4]
            if rational:
                den = t[4] if len(t) == 5 else [1] * len(val)
                a = ((ctypes.c_uint32 * len(rowptr))(*rowptr), (ctypes.c_uint32 * max(len(col), 1))(*col), (ctypes.c_int64 * max(len(val), 1))(*[int(x) for x in val]),
                     (ctypes.c_int64 * max(len(den), 1))(*[int(x) for x in den]))
                cs.append(capi.QCSR(m, n, a[0], a[1], a[2], a[3]))
            else:
                a = ((ctypes.c_uint32 * len(rowptr))(*rowptr), (ctypes.c_uint32 * max(len(col), 1))(*col), (ctypes.c_int32 * max(len(val), 1))(*val))
                cs.append(capi.ICSR(m, n, a[0], a[1], a[2]))
            self._keep.append(a)
        self._h = ctypes.c_void_p()
        create = L.plo_tril_plan_create_q if rational else L.plo_tril_plan_create_x
        capi.check(create(ctypes.byref(cs[0]), ctypes.byref(cs[1]), ctypes.byref(cs[2]), int(bool(expanded)), ctypes.byref(self._h)))
        self.last_stats = None

    def __del__(self):
        try:
            if self._h:
                capi.lib().plo_tril_plan_destroy(self._h); self._h = None
        except Exception:
            pass

    def cost_many(self, seeds=None, seed0=0, n=0):
        L = capi.lib()
        if seeds is not None:
            n = len(seeds); sp = (ctypes.c_uint64 * max(n, 1))(*seeds)
        else:
            sp = None
        ops = (ctypes.c_uint32 * (6 * max(n, 1)))()
        st = capi.Stats()
        capi.check(L.plo_tril_cost_many(self._h, sp, seed0, n, ops, ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return [(tuple(ops[6 * k:6 * k + 3]), tuple(ops[6 * k + 3:6 * k + 6])) for k in range(n)]

    def search(self, seed0, nseeds):
        b, st = capi.TrilBest(), capi.Stats()
        capi.check(capi.lib().plo_tril_search(self._h, seed0, nseeds, ctypes.byref(b), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return (b.add, b.sca, b.mul), b.seed, b.variant


LIN_BASE_SEED = (1 << 64) - 1


def _qcsr(m, n, rowptr, col, num, den):
    den = [1] * len(num) if den is None else den
    a = ((ctypes.c_uint32 * len(rowptr))(*rowptr), (ctypes.c_uint32 * max(len(col), 1))(*col), (ctypes.c_int64 * max(len(num), 1))(*[int(x) for x in num]),
         (ctypes.c_int64 * max(len(den), 1))(*[int(x) for x in den]))
    return capi.QCSR(m, n, a[0], a[1], a[2], a[3]), a


class LinPlan:
    """Mirror of the restart loop of `SearchLinearAlgorithm` (reference include/plinopt_inplace.inl:604-673, bin/inplacer):
    A (m x n) as a rational CSR (rowptr, col, num[, den]); empty rows allowed.  `cost_many` returns, per seed,
    ((ADD,SCA,ROWS) of variant 0 = unoriented, (ADD,SCA,ROWS) of variant 1 = oriented appended to variant 0);
    `search` the best ((ADD, SCA, ROWS), seed, variant) under the reference's order (:637-641), ties to the smaller
    (seed, variant).  LIN_BASE_SEED is the unpermuted oriented program of :613."""

    def __init__(self, m, n, rowptr, col, num, den=None, device=None):
        L = capi.lib()
        if device is not None:
            capi.check(L.plo_init(device))
        self._h = None
        self._csr, self._keep = _qcsr(m, n, rowptr, col, num, den)
        h = ctypes.c_void_p()
        capi.check(L.plo_lin_plan_create_q(ctypes.byref(self._csr), ctypes.byref(h)))
        self._h = h
        self.last_stats = None

    def __del__(self):
        try:
            if self._h:
                capi.lib().plo_lin_plan_destroy(self._h); self._h = None
        except Exception:
            pass

    def cost_many(self, seeds=None, seed0=0, n=0):
        L = capi.lib()
        if seeds is not None:
            n = len(seeds); sp = (ctypes.c_uint64 * max(n, 1))(*seeds)
        else:
            sp = None
        ops = (ctypes.c_uint32 * (6 * max(n, 1)))()
        st = capi.Stats()
        capi.check(L.plo_lin_cost_many(self._h, sp, seed0, n, ops, ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return [(tuple(ops[6 * k:6 * k + 3]), tuple(ops[6 * k + 3:6 * k + 6])) for k in range(n)]

    def search(self, seed0, nseeds):
        b, st = capi.LinBest(), capi.Stats()
        capi.check(capi.lib().plo_lin_search(self._h, seed0, nseeds, ctypes.byref(b), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return (b.add, b.sca, b.rows), b.seed, b.variant


def lin_search_multi(m, n, rowptr, col, num, den, seed0, nseeds, devices):
    """`plo_lin_search_multi`: the restart loop of SearchLinearAlgorithm over the listed devices from this process.
    Returns (((ADD, SCA, ROWS), seed, variant), stats)."""
    L = capi.lib()
    csr, keep = _qcsr(m, n, rowptr, col, num, den)
    dv = (ctypes.c_int * len(devices))(*devices)
    b, st = capi.LinBest(), capi.Stats()
    capi.check(L.plo_lin_search_multi(ctypes.byref(csr), seed0, nseeds, len(devices), dv, ctypes.byref(b), ctypes.byref(st)))
    del keep
    return ((b.add, b.sca, b.rows), b.seed, b.variant), st.as_dict()


ORBIT_BASE_SEED = (1 << 64) - 1
ORBIT_DENSITY, ORBIT_CSE, ORBIT_CANONICAL, ORBIT_GROWTH = 0, 1, 2, 3
ORBIT_ACT_TRIANGULAR, ORBIT_ACT_PLUQ, ORBIT_ACT_HOUSEHOLDER = 0, 1, 2


class OrbitPlan:
    """Mirror of the restart loop of the reference's orbiter (src/orbiter.cpp:272-324, bin/orbiter): the triple L (r x mk),
    R (r x kn), P (mn x r), each as a rational CSR (m, n, rowptr, col, num[, den]), over Q (modulus 0) or Z_modulus
    (< 2^31), scored by `measure` (ORBIT_DENSITY or ORBIT_CANONICAL).  `cost_many` returns (cost, nnz, nno) per seed;
    `search` the best ((cost, nnz, nno), seed), ties to the smaller seed.  ORBIT_BASE_SEED is the input itself.  `action`
    (ORBIT_ACT_TRIANGULAR, ORBIT_ACT_PLUQ or ORBIT_ACT_HOUSEHOLDER) is how U, V and W are drawn.  measure=ORBIT_CSE
    (`plo_orbit_plan_create_cse`, bin/orbiter -z; an odd prime modulus) scores a candidate by the operations of the best
    programs found for its three matrices: per matrix the minimum of naiveOps and of `sub` Optimizer runs with the streams
    cse_seed0 .. cse_seed0 + sub - 1.  `info()` is `plo_orbit_plan_info`."""

    def __init__(self, L, R, P, modulus=0, measure=ORBIT_DENSITY, device=None, action=ORBIT_ACT_TRIANGULAR, sub=1, cse_seed0=0):
        lib = capi.lib()
        if device is not None:
            capi.check(lib.plo_init(device))
        self._h = None
        self._csr = [_qcsr(*(tuple(A) + (None,) * (6 - len(A)))) for A in (L, R, P)]
        h = ctypes.c_void_p()
        if measure == ORBIT_CSE:
            capi.check(lib.plo_orbit_plan_create_cse(*[ctypes.byref(c) for c, _ in self._csr], modulus, action, sub, cse_seed0, ctypes.byref(h)))
        else:
            capi.check(lib.plo_orbit_plan_create_act(*[ctypes.byref(c) for c, _ in self._csr], modulus, measure, action, ctypes.byref(h)))
        self._h = h
        self.last_stats = None

    def __del__(self):
        try:
            if self._h:
                capi.lib().plo_orbit_plan_destroy(self._h); self._h = None
        except Exception:
            pass

    def cost_many(self, seeds=None, seed0=0, n=0):
        lib = capi.lib()
        if seeds is not None:
            n = len(seeds); sp = (ctypes.c_uint64 * max(n, 1))(*seeds)
        else:
            sp = None
        out = (ctypes.c_uint32 * (3 * max(n, 1)))()
        st = capi.Stats()
        capi.check(lib.plo_orbit_cost_many(self._h, sp, seed0, n, out, ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return [tuple(out[3 * k:3 * k + 3]) for k in range(n)]

    def search(self, seed0, nseeds):
        b, st = capi.OrbitBest(), capi.Stats()
        capi.check(capi.lib().plo_orbit_search(self._h, seed0, nseeds, ctypes.byref(b), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return (b.cost, b.nnz, b.nno), b.seed

    def info(self):
        out = (ctypes.c_uint32 * 8)()
        capi.check(capi.lib().plo_orbit_plan_info(self._h, out))
        return {"waves_per_wg": out[0], "lds_bytes": out[1], "table_slots": tuple(out[2:5]), "entry_bound": out[5], "relaunches": out[6], "keeps_whole_image": bool(out[7])}


def orbit_search_multi(L, R, P, modulus, measure, seed0, nseeds, devices, action=ORBIT_ACT_TRIANGULAR, sub=1, cse_seed0=0):
    """`plo_orbit_search_multi_act` (`plo_orbit_search_multi_cse` for measure=ORBIT_CSE): the orbit search over the listed devices
    from this process (L, R, P as for OrbitPlan).  Returns (((cost, nnz, nno), seed), stats)."""
    lib = capi.lib()
    csr = [_qcsr(*(tuple(A) + (None,) * (6 - len(A)))) for A in (L, R, P)]
    dv = (ctypes.c_int * len(devices))(*devices)
    b, st = capi.OrbitBest(), capi.Stats()
    if measure == ORBIT_CSE:
        capi.check(lib.plo_orbit_search_multi_cse(*[ctypes.byref(c) for c, _ in csr], modulus, action, sub, cse_seed0, seed0, nseeds, len(devices), dv, ctypes.byref(b), ctypes.byref(st)))
    else:
        capi.check(lib.plo_orbit_search_multi_act(*[ctypes.byref(c) for c, _ in csr], modulus, measure, action, seed0, nseeds, len(devices), dv, ctypes.byref(b), ctypes.byref(st)))
    del csr
    return ((b.cost, b.nnz, b.nno), b.seed), st.as_dict()


class OrbitGrowthPlan(OrbitPlan):
    """The orbit search scored by the 2-norm growth factor (`plo_orbit_plan_create_growth`, bin/orbiter -g; PLO_ORBIT_GROWTH of
    include/plinopt_hip.h): over Q, action ORBIT_ACT_TRIANGULAR or ORBIT_ACT_PLUQ.  `growth_many` returns (cost, nnz, nno) per
    seed, the cost a float whose bits are part of the definition; `growth_search` the best ((cost, nnz, nno), seed) under
    (bits of the cost, nnz, nno, seed).  `cost_many` and `search` of the parent raise PLO_E_ARG on such a plan."""

    def __init__(self, L, R, P, device=None, action=ORBIT_ACT_TRIANGULAR):
        lib = capi.lib()
        if device is not None:
            capi.check(lib.plo_init(device))
        self._h = None
        self._csr = [_qcsr(*(tuple(A) + (None,) * (6 - len(A)))) for A in (L, R, P)]
        h = ctypes.c_void_p()
        capi.check(lib.plo_orbit_plan_create_growth(*[ctypes.byref(c) for c, _ in self._csr], action, ctypes.byref(h)))
        self._h = h
        self.last_stats = None

    def growth_many(self, seeds=None, seed0=0, n=0):
        lib = capi.lib()
        if seeds is not None:
            n = len(seeds); sp = (ctypes.c_uint64 * max(n, 1))(*seeds)
        else:
            sp = None
        cost = (ctypes.c_double * max(n, 1))()
        cnt = (ctypes.c_uint32 * (2 * max(n, 1)))()
        st = capi.Stats()
        capi.check(lib.plo_orbit_growth_many(self._h, sp, seed0, n, cost, cnt, ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return [(cost[k], cnt[2 * k], cnt[2 * k + 1]) for k in range(n)]

    def growth_search(self, seed0, nseeds):
        b, st = capi.OrbitGBest(), capi.Stats()
        capi.check(capi.lib().plo_orbit_growth_search(self._h, seed0, nseeds, ctypes.byref(b), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return (b.cost, b.nnz, b.nno), b.seed


def orbit_growth_search_multi(L, R, P, seed0, nseeds, devices, action=ORBIT_ACT_TRIANGULAR):
    """`plo_orbit_growth_search_multi`: the growth-factor orbit search over the listed devices from this process.
    Returns (((cost, nnz, nno), seed), stats)."""
    lib = capi.lib()
    csr = [_qcsr(*(tuple(A) + (None,) * (6 - len(A)))) for A in (L, R, P)]
    dv = (ctypes.c_int * len(devices))(*devices)
    b, st = capi.OrbitGBest(), capi.Stats()
    capi.check(lib.plo_orbit_growth_search_multi(*[ctypes.byref(c) for c, _ in csr], action, seed0, nseeds, len(devices), dv, ctypes.byref(b), ctypes.byref(st)))
    del csr
    return ((b.cost, b.nnz, b.nno), b.seed), st.as_dict()


DEP_ZERO, DEP_ONE = 0, 1
DEP_PRIME = 2147483629


class DepPlan:
    """Mirror of the enumeration of the reference's `dependency` (src/dependency.cpp:74-101, 158-165, bin/dependency): M (m x n)
    as a rational CSR (rowptr, col, num[, den]), the coefficient list as (numerator, denominator) pairs, over Q (modulus 0) or
    Z_modulus (< 2^31), combinations of at most `level` rows (1 .. 8).  `search` returns the hits of the top rows
    [row0, row1) in the reference's depth-first order, each (rows, coefficient indices, kind, column, residue): the top row has
    coefficient 1 and index None.  Over Q the device works modulo DEP_PRIME and the list is a superset of the true hits: the
    caller recomputes every combination over Q.  More hits than `cap` raise PloError(PLO_E_CAPACITY) with the full count in
    `last_nhits`."""

    def __init__(self, m, n, rowptr, col, num, den=None, coeffs=((1, 1), (-1, 1)), modulus=0, level=4, device=None):
        L = capi.lib()
        if device is not None:
            capi.check(L.plo_init(device))
        self._h = None
        self._csr, self._keep = _qcsr(m, n, rowptr, col, num, den)
        cn = (ctypes.c_int64 * max(len(coeffs), 1))(*[int(c[0]) for c in coeffs])
        cd = (ctypes.c_int64 * max(len(coeffs), 1))(*[int(c[1]) for c in coeffs])
        h = ctypes.c_void_p()
        capi.check(L.plo_dep_plan_create_q(ctypes.byref(self._csr), cn, cd, len(coeffs), modulus, level, ctypes.byref(h)))
        self._h = h
        self.m = m
        self.last_stats = None
        self.last_nhits = None

    def __del__(self):
        try:
            if self._h:
                capi.lib().plo_dep_plan_destroy(self._h); self._h = None
        except Exception:
            pass

    def search(self, row0=0, row1=None, cap=1 << 16):
        row1 = self.m if row1 is None else row1
        hits = (capi.DepHit * max(cap, 1))()
        nh, st = ctypes.c_uint64(0), capi.Stats()
        rc = capi.lib().plo_dep_search(self._h, row0, row1, hits, cap, ctypes.byref(nh), ctypes.byref(st))
        self.last_nhits = nh.value
        capi.check(rc)
        self.last_stats = st.as_dict()
        return [(tuple(h.rows[:h.size]), (None,) + tuple(h.coef[1:h.size]), h.kind, h.col, h.residue) for h in hits[:nh.value]]


class BrentPlan:
    """Mirror of the exact matrix-multiplication check of bin/MMchecker (plo_brent_*): L (r x mk), R (r x kn), P (mn x r), each
    (rows, columns, rowptr, col, num[, den]), and the shape (m, k, n); every Brent equation modulo q (2 <= q < 2^31, prime or
    not).  `check(pair0, pair1)` covers the pairs x kn + y of [pair0, pair1) (default: all) and returns (violated, first,
    value, expected): the number of violated equations, the smallest one e = (x kn + y) mn + z (None when there is none), the
    residue found there and the 0 or 1 it should be.  `info()` is `plo_brent_plan_info`."""

    def __init__(self, L, R, P, m, k, n, q, device=None):
        lib = capi.lib()
        if device is not None:
            capi.check(lib.plo_init(device))
        self._h = None
        self._csr = [_qcsr(*(tuple(A) + (None,) * (6 - len(A)))) for A in (L, R, P)]
        h = ctypes.c_void_p()
        capi.check(lib.plo_brent_plan_create_q(*[ctypes.byref(c) for c, _ in self._csr], m, k, n, q, ctypes.byref(h)))
        self._h = h
        self.npairs = m * k * k * n
        self.last_stats = None

    def __del__(self):
        try:
            if self._h:
                capi.lib().plo_brent_plan_destroy(self._h); self._h = None
        except Exception:
            pass

    def info(self):
        out = (ctypes.c_uint32 * 8)()
        capi.check(capi.lib().plo_brent_plan_info(self._h, out))
        return dict(zip(("chunk", "chunks", "waves_per_wg", "pairs_per_launch", "lds_bytes", "mk", "kn", "mn"), out))

    def check(self, pair0=0, pair1=None):
        res, st = capi.BrentResult(), capi.Stats()
        capi.check(capi.lib().plo_brent_check(self._h, pair0, self.npairs if pair1 is None else pair1, ctypes.byref(res), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return res.violated, (res.first if res.violated else None), res.value, res.expected


class PolyMulPlan:
    """Mirror of the exact polynomial-multiplication check of bin/PMchecker (plo_polymul_*): L (r x na), R (r x nb), P (nc x r),
    each (rows, columns, rowptr, col, num[, den]), modulo q (2 <= q < 2^31, prime or not), and optionally the polynomial `f` as
    its coefficients, constant term first, each an integer or a (numerator, denominator) pair.  `check(pair0, pair1)` covers
    the pairs i nb + j of [pair0, pair1) (default: all) and returns (violated, first, value, expected): the number of violated
    equations, the smallest one e = (i nb + j) w + c (None when there is none), the residue found there and the one it should
    be; w is max(nc, na + nb - 1) without f and its degree with it.  `info()` is `plo_polymul_plan_info`."""

    def __init__(self, L, R, P, q, f=None, device=None):
        lib = capi.lib()
        if device is not None:
            capi.check(lib.plo_init(device))
        self._h = None
        self._csr = [_qcsr(*(tuple(A) + (None,) * (6 - len(A)))) for A in (L, R, P)]
        f = [c if isinstance(c, (tuple, list)) else (c, 1) for c in (f or [])]
        fn = (ctypes.c_int64 * max(len(f), 1))(*[int(c[0]) for c in f])
        fd = (ctypes.c_int64 * max(len(f), 1))(*[int(c[1]) for c in f])
        h = ctypes.c_void_p()
        capi.check(lib.plo_polymul_plan_create_q(*[ctypes.byref(c) for c, _ in self._csr], fn, fd, len(f), q, ctypes.byref(h)))
        self._h = h
        self.npairs = L[1] * R[1]
        self.last_stats = None

    def __del__(self):
        try:
            if self._h:
                capi.lib().plo_polymul_plan_destroy(self._h); self._h = None
        except Exception:
            pass

    def info(self):
        out = (ctypes.c_uint32 * 8)()
        capi.check(capi.lib().plo_polymul_plan_info(self._h, out))
        return dict(zip(("chunk", "chunks", "waves_per_wg", "pairs_per_launch", "lds_bytes", "npairs", "w", "fold"), out))

    def check(self, pair0=0, pair1=None):
        res, st = capi.BrentResult(), capi.Stats()
        capi.check(capi.lib().plo_polymul_check(self._h, pair0, self.npairs if pair1 is None else pair1, ctypes.byref(res), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return res.violated, (res.first if res.violated else None), res.value, res.expected


class TProgPlan:
    """Mirror of the exact check of an in-place trilinear program of bin/TPchecker (plo_tprog_*): L (r x na), R (r x nb),
    P (nc0 x r), each (rows, columns, rowptr, col, num[, den]), the program as records (family, op, part, dst, src, src2, num,
    den) -- family 0 a, 1 b, 2 c; op 0 ADD, 1 SCA, 2 AXPY; part 0, or 1 low / 2 hig with `expanded` -- modulo q (2 <= q < 2^31,
    prime or not).  `matmul`: the target is the matrix-multiplication tensor of the shape.  `check(pair0, pair1)` covers the
    bilinear equations of the pairs i nb + j of [pair0, pair1) (default: all) and, from pair 0, the restoration blocks A, B, C
    behind them; it returns (violated, first, value, expected) under the numbering of DESIGN.md 2.14 (first None when there
    is none).  `info()` is `plo_tprog_plan_info`."""
    EXPANDED, MATMUL = 1, 2

    def __init__(self, L, R, P, records, q, expanded=False, matmul=False, device=None):
        lib = capi.lib()
        if device is not None:
            capi.check(lib.plo_init(device))
        self._h = None
        self._csr = [_qcsr(*(tuple(A) + (None,) * (6 - len(A)))) for A in (L, R, P)]
        recs = (capi.TProgRec * max(len(records), 1))()
        for k, (fam, op, part, dst, src, src2, num, den) in enumerate(records):
            recs[k] = capi.TProgRec(fam, op, part, 0, dst, src, src2, num, den)
        h = ctypes.c_void_p()
        flags = (self.EXPANDED if expanded else 0) | (self.MATMUL if matmul else 0)
        capi.check(lib.plo_tprog_plan_create_q(*[ctypes.byref(c) for c, _ in self._csr], recs, len(records), flags, q, ctypes.byref(h)))
        self._h = h
        self.npairs = L[1] * R[1]
        self.last_stats = None

    def __del__(self):
        try:
            if self._h:
                capi.lib().plo_tprog_plan_destroy(self._h); self._h = None
        except Exception:
            pass

    def info(self):
        out = (ctypes.c_uint32 * 8)()
        capi.check(capi.lib().plo_tprog_plan_info(self._h, out))
        return dict(zip(("max_words", "lds_words_per_wave", "waves_per_wg", "waves_per_launch", "records", "npairs", "w", "rows"), out))

    def check(self, pair0=0, pair1=None):
        res, st = capi.BrentResult(), capi.Stats()
        capi.check(capi.lib().plo_tprog_check(self._h, pair0, self.npairs if pair1 is None else pair1, ctypes.byref(res), ctypes.byref(st)))
        self.last_stats = st.as_dict()
        return res.violated, (res.first if res.violated else None), res.value, res.expected
