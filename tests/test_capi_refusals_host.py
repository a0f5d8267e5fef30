"""What every C-API entry answers before it touches a device: for each call of a table, the return code and, where the
call fails, the text of plo_last_error(), against tests/golden/capi_refusals.json.  The tools print these texts and tests
compare tool output; the ORDER of an entry's checks is part of what is pinned (atoms_search and cost_many_run look for
the device before their arguments, the CSE entries after them).  A call that succeeds or returns nothing sets no text:
its row holds null there.

One fresh child process walks the table through ctypes.  It never calls plo_init and imports no torch, so it answers
the same with and without a GPU.  Entries that take a plan get a zeroed buffer in its place where the refusal comes
before the plan is read (the missing-plo_init refusals, the growth/non-growth mismatch).

Not reachable without a device, and therefore not here: the csr_defect / qcsr_defect / trilmat_check texts, the orbit
shape and action checks and the per-call candidate counts of the single-device searches all sit behind the entry's
device check (or behind the plo_init(0) that plo_cse_plan_create_ex and the change-of-basis entries make themselves).

PLO_HIP_LIB names another build of the library, as for plinopt_amd.capi.
Regenerate: python tests/test_capi_refusals_host.py --record
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "capi_refusals.json")
LIB = os.environ.get("PLO_HIP_LIB") or os.path.join(ROOT, "plinopt_amd", "libplinopt_hip.so")

u32, u64, i32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
u32p = ctypes.POINTER(u32)


class CSR(ctypes.Structure):
    _fields_ = [("m", u32), ("n", u32), ("rowptr", u32p), ("col", u32p), ("val", u32p)]


class ICSR(ctypes.Structure):
    _fields_ = [("m", u32), ("n", u32), ("rowptr", u32p), ("col", u32p), ("val", ctypes.POINTER(ctypes.c_int32))]


class QCSR(ctypes.Structure):
    _fields_ = [("m", u32), ("n", u32), ("rowptr", u32p), ("col", u32p), ("num", ctypes.POINTER(ctypes.c_int64)), ("den", ctypes.POINTER(ctypes.c_int64))]


class CobProblem(ctypes.Structure):
    _fields_ = [("TM", u32p), ("Cand", u32p), ("coeffs", u32p), ("ncoeffs", u32), ("p", u32), ("w0", ctypes.c_int32), ("w1", ctypes.c_int32)]


def calls(L):
    """(label, function, arguments) of every call, in the order they are made"""
    ref = ctypes.byref
    one = (u32 * 1)(1)
    rp, col, val = (u32 * 2)(0, 1), (u32 * 1)(0), (u32 * 1)(1)
    A = CSR(1, 1, rp, col, val)                                     # the 1 x 1 matrix (1)
    nullrp = CSR(1, 1, None, None, None)
    I = ICSR(1, 1, rp, col, (ctypes.c_int32 * 1)(1))
    Inull = ICSR(1, 1, None, None, None)
    Q = QCSR(1, 1, rp, col, (ctypes.c_int64 * 1)(1), None)
    fake = ctypes.create_string_buffer(1 << 16)                     # a plan that is never read (or read as zeros: no growth plan)
    h = ctypes.c_void_p()
    out = ctypes.create_string_buffer(256)                          # any result structure
    words = (u32 * 16)()
    w64 = (u64 * 4)()
    dbl = (ctypes.c_double * 2)()
    devs = (i32 * 2)(0, 0)
    prob_ok = CobProblem(one, one, one, 1, 7, 0, 0)
    prob4 = (CobProblem * 4)(prob_ok, prob_ok, prob_ok, CobProblem(one, one, one, 1, 8, 0, 0))

    def cob_range(n=2, m=2, TM=one, Cand=one, row=0, blk=0, cf=one, nc=1, p=7, first=0, ngroups=1, o=out):
        return ("plo_cob_search_range", L.plo_cob_search_range, (u32(n), u32(m), TM, Cand, u32(row), u32(blk), cf, u32(nc), u32(p), i32(0), i32(0), u64(first), u64(ngroups), o, None))

    T = []

    def add(label, name, *args):
        T.append((label, getattr(L, name), args))

    add("shutdown without init", "plo_shutdown")
    add("multi_comm_inits", "plo_multi_comm_inits")
    add("pack_cost mode 0", "plo_pack_cost", u32(10), u32(2), i32(0), u32(7))
    add("pack_cost mode 1", "plo_pack_cost", u32(10), u32(2), i32(1), u32(7))
    add("pack_cost mode 2", "plo_pack_cost", u32(10), u32(2), i32(2), u32(7))
    # ---- CSE plans
    add("plan_create: null matrix", "plo_cse_plan_create", None, u32(7), ref(h))
    add("plan_create: null out", "plo_cse_plan_create", ref(A), u32(7), None)
    add("plan_create: null rowptr", "plo_cse_plan_create", ref(nullrp), u32(7), ref(h))
    add("plan_create: even modulus", "plo_cse_plan_create", ref(A), u32(4), ref(h))
    add("plan_create: modulus 1", "plo_cse_plan_create", ref(A), u32(1), ref(h))
    add("plan_create: modulus 2^31", "plo_cse_plan_create", ref(A), u32(1 << 31), ref(h))
    add("plan_create_ex: null matrix", "plo_cse_plan_create_ex", None, u32(7), u32(1), ref(h))
    add("plan_create_ex: even modulus", "plo_cse_plan_create_ex", ref(A), u32(6), u32(1), ref(h))
    add("plan_is_hbm: null", "plo_cse_plan_is_hbm", None)
    add("hbm_info: null", "plo_cse_plan_hbm_info", None, words)
    add("hbm_info: null out", "plo_cse_plan_hbm_info", fake, None)
    add("hbm_info: no HBM plan", "plo_cse_plan_hbm_info", fake, words)
    add("hbm_counters: null", "plo_cse_plan_hbm_counters", None, words)
    add("hbm_counters_ex: null", "plo_cse_plan_hbm_counters_ex", None, words, u32(8))
    add("hbm_counters_ex: n = 14", "plo_cse_plan_hbm_counters_ex", fake, words, u32(14))
    add("hbm_workspace_layout: 9 table bits", "plo_cse_hbm_workspace_layout", u32(4), u32(8), u32(16), u32(9), w64)
    add("hbm_workspace_layout: null out", "plo_cse_hbm_workspace_layout", u32(4), u32(8), u32(16), u32(10), None)
    add("hbm_workspace_layout: host only", "plo_cse_hbm_workspace_layout", u32(4), u32(8), u32(16), u32(10), w64)
    add("plan_destroy: null", "plo_cse_plan_destroy", None)
    add("cost_many_plan: null plan", "plo_cse_cost_many_plan", None, None, u64(0), u64(1), words, words, None)
    add("cost_many_plan: null adds", "plo_cse_cost_many_plan", fake, None, u64(0), u64(1), None, words, None)
    add("cost_many_plan: no plo_init", "plo_cse_cost_many_plan", fake, None, u64(0), u64(1), words, words, None)
    add("cost_many: null matrix", "plo_cse_cost_many", None, u32(7), None, u64(0), u64(1), words, words)
    add("cost_many: even modulus", "plo_cse_cost_many", ref(A), u32(10), None, u64(0), u64(1), words, words)
    add("search_plan: null plan", "plo_cse_search_plan", None, u64(0), u64(1), i32(0), out, None)
    add("search_plan: null out", "plo_cse_search_plan", fake, u64(0), u64(1), i32(0), None, None)
    add("search_plan: cost mode 3", "plo_cse_search_plan", fake, u64(0), u64(1), i32(3), out, None)
    add("search_plan: cost mode -1", "plo_cse_search_plan", fake, u64(0), u64(1), i32(-1), out, None)
    add("search_plan: no plo_init", "plo_cse_search_plan", fake, u64(0), u64(1), i32(0), out, None)
    add("search: null matrix", "plo_cse_search", None, u32(7), u64(0), u64(1), i32(0), out, None)
    add("search: modulus 2", "plo_cse_search", ref(A), u32(2), u64(0), u64(1), i32(0), out, None)
    add("enum_cost_many_plan: null plan", "plo_cse_enum_cost_many_plan", None, u64(0), u64(1), words, words, None, None)
    add("enum_cost_many_plan: no plo_init", "plo_cse_enum_cost_many_plan", fake, u64(0), u64(1), words, words, None, None)
    add("enum_search_plan: null maxprod", "plo_cse_enum_search_plan", fake, u64(0), u64(1), i32(0), out, None, None)
    add("enum_search_plan: cost mode 2", "plo_cse_enum_search_plan", fake, u64(0), u64(1), i32(2), out, w64, None)
    add("enum_search_plan: no plo_init", "plo_cse_enum_search_plan", fake, u64(0), u64(1), i32(3), out, w64, None)
    # ---- chained CSE
    add("chain_destroy: null", "plo_cse_chain_destroy", None)
    add("chain_create: null second", "plo_cse_chain_create", ref(A), None, u32(7), ref(h))
    add("chain_create: null out", "plo_cse_chain_create", ref(A), ref(A), u32(7), None)
    add("chain_create: even modulus", "plo_cse_chain_create", ref(A), ref(A), u32(8), ref(h))
    add("chain_batch: null firsts", "plo_cse_chain_batch", u32(1), None, ref(A), u32(7), u64(0), u32(1), i32(0), None, None, out, None)
    add("chain_batch: no pairs", "plo_cse_chain_batch", u32(0), ref(A), ref(A), u32(7), u64(0), u32(1), i32(0), None, None, out, None)
    add("chain_batch: per_pair 0", "plo_cse_chain_batch", u32(1), ref(A), ref(A), u32(7), u64(0), u32(0), i32(0), None, None, out, None)
    add("chain_batch: cost mode 3", "plo_cse_chain_batch", u32(1), ref(A), ref(A), u32(7), u64(0), u32(1), i32(3), None, None, out, None)
    add("chain_batch: no plo_init", "plo_cse_chain_batch", u32(1), ref(A), ref(A), u32(7), u64(0), u32(1), i32(0), None, None, out, None)
    add("chain_batch: no plo_init comes before the modulus", "plo_cse_chain_batch", u32(1), ref(A), ref(A), u32(4), u64(0), u32(1), i32(0), None, None, out, None)
    add("chain_cost_many: null chain", "plo_cse_chain_cost_many", None, None, u64(0), u64(1), words, words, None)
    add("chain_cost_many: null muls", "plo_cse_chain_cost_many", fake, None, u64(0), u64(1), words, None, None)
    add("chain_cost_many: nothing to do", "plo_cse_chain_cost_many", fake, None, u64(0), u64(0), words, words, None)
    add("chain_search: null chain", "plo_cse_chain_search", None, u64(0), u64(1), i32(0), out, None)
    add("chain_search: null out", "plo_cse_chain_search", fake, u64(0), u64(1), i32(0), None, None)
    add("chain_search: cost mode 3", "plo_cse_chain_search", fake, u64(0), u64(1), i32(3), out, None)
    # ---- kernel method
    add("kernel_search: null matrix", "plo_kernel_search", None, u32(7), u64(0), u64(1), u32(1), i32(0), None, None, None, out, None)
    add("kernel_search: no restarts", "plo_kernel_search", ref(A), u32(7), u64(0), u64(0), u32(1), i32(0), None, None, None, out, None)
    add("kernel_search: per_block 0", "plo_kernel_search", ref(A), u32(7), u64(0), u64(1), u32(0), i32(0), None, None, None, out, None)
    add("kernel_search: cost mode 3", "plo_kernel_search", ref(A), u32(7), u64(0), u64(1), u32(1), i32(3), None, None, None, out, None)
    add("kernel_search: no plo_init", "plo_kernel_search", ref(A), u32(7), u64(0), u64(1), u32(1), i32(0), None, None, None, out, None)
    add("kernel_search: no plo_init comes before the modulus", "plo_kernel_search", ref(A), u32(4), u64(0), u64(1), u32(1), i32(0), None, None, None, out, None)
    # ---- one process, N devices
    add("cse_search_multi: null matrix", "plo_cse_search_multi", None, u32(7), u64(0), u64(1), i32(0), i32(1), None, out, None)
    add("cse_search_multi: no device", "plo_cse_search_multi", ref(A), u32(7), u64(0), u64(1), i32(0), i32(0), None, out, None)
    add("cse_search_multi: 65 devices", "plo_cse_search_multi", ref(A), u32(7), u64(0), u64(1), i32(0), i32(65), None, out, None)
    add("cse_search_multi: cost mode 3", "plo_cse_search_multi", ref(A), u32(7), u64(0), u64(1), i32(3), i32(1), None, out, None)
    add("kernel_search_multi: null out", "plo_kernel_search_multi", ref(A), u32(7), u64(0), u64(1), u32(1), i32(0), i32(1), None, None, None)
    add("kernel_search_multi: 65 devices", "plo_kernel_search_multi", ref(A), u32(7), u64(0), u64(1), u32(1), i32(0), i32(65), None, out, None)
    add("kernel_search_multi: cost mode 3", "plo_kernel_search_multi", ref(A), u32(7), u64(0), u64(1), u32(1), i32(3), i32(1), None, out, None)
    add("kernel_search_multi: per_block 2 on two devices", "plo_kernel_search_multi", ref(A), u32(7), u64(0), u64(2), u32(2), i32(0), i32(2), devs, out, None)
    add("tril_search_multi: null T", "plo_tril_search_multi", ref(Q), ref(Q), None, i32(0), u64(0), u64(1), i32(1), None, out, None)
    add("tril_search_multi: no device", "plo_tril_search_multi", ref(Q), ref(Q), ref(Q), i32(0), u64(0), u64(1), i32(0), None, out, None)
    add("tril_search_multi: no candidate", "plo_tril_search_multi", ref(Q), ref(Q), ref(Q), i32(0), u64(0), u64(0), i32(1), None, out, None)
    add("tril_search_multi: 2^62 candidates", "plo_tril_search_multi", ref(Q), ref(Q), ref(Q), i32(0), u64(0), u64(1 << 62), i32(1), None, out, None)
    add("lin_search_multi: null best", "plo_lin_search_multi", ref(Q), u64(0), u64(1), i32(1), None, None, None)
    add("lin_search_multi: 65 devices", "plo_lin_search_multi", ref(Q), u64(0), u64(1), i32(65), None, out, None)
    add("lin_search_multi: no candidate", "plo_lin_search_multi", ref(Q), u64(0), u64(0), i32(1), None, out, None)
    add("orbit_search_multi: null L", "plo_orbit_search_multi", None, ref(Q), ref(Q), u64(0), i32(0), u64(0), u64(1), i32(1), None, out, None)
    add("orbit_search_multi: no device", "plo_orbit_search_multi", ref(Q), ref(Q), ref(Q), u64(0), i32(0), u64(0), u64(1), i32(0), None, out, None)
    add("orbit_search_multi_act: no candidate", "plo_orbit_search_multi_act", ref(Q), ref(Q), ref(Q), u64(0), i32(0), i32(1), u64(0), u64(0), i32(1), None, out, None)
    add("orbit_search_multi_cse: null best", "plo_orbit_search_multi_cse", ref(Q), ref(Q), ref(Q), u64(7), i32(0), u32(1), u64(0), u64(0), u64(1), i32(1), None, None, None)
    add("orbit_search_multi_cse: 2^31 candidates on 65 devices", "plo_orbit_search_multi_cse", ref(Q), ref(Q), ref(Q), u64(7), i32(0), u32(1), u64(0), u64(0), u64(1 << 31), i32(65), None, out, None)
    add("orbit_growth_search_multi: null P", "plo_orbit_growth_search_multi", ref(Q), ref(Q), None, i32(0), u64(0), u64(1), i32(1), None, out, None)
    add("orbit_growth_search_multi: no candidate", "plo_orbit_growth_search_multi", ref(Q), ref(Q), ref(Q), i32(0), u64(0), u64(0), i32(1), None, out, None)
    # ---- change of basis (nothing here gets past cob_check: the entries call plo_init(0) themselves)
    T.append(cob_range(o=None))
    T.append(cob_range(TM=None))
    T.append(cob_range(p=4))
    T.append(cob_range(p=1))
    T.append(cob_range(n=0))
    T.append(cob_range(row=2))
    T.append(cob_range(blk=2))
    T.append(cob_range(nc=0))
    T.append(cob_range(nc=256))
    T.append(cob_range(n=65535, m=65536))
    add("cob_search: null coefficients", "plo_cob_search", u32(2), u32(2), one, one, u32(0), u32(0), None, u32(1), u32(7), i32(0), i32(0), out, None)
    add("cob_search: even modulus", "plo_cob_search", u32(2), u32(2), one, one, u32(0), u32(0), one, u32(1), u32(2), i32(0), i32(0), out, None)
    T.append(cob_range(nc=2, first=9))
    T.append(cob_range(nc=2, first=4, ngroups=5))
    add("cob_search_batch: no enumeration", "plo_cob_search_batch", u32(0), u32(2), u32(2), u32(0), u32(0), prob4, out, None)
    add("cob_search_batch: five enumerations", "plo_cob_search_batch", u32(5), u32(2), u32(2), u32(0), u32(0), prob4, out, None)
    add("cob_search_batch: null problems", "plo_cob_search_batch", u32(1), u32(2), u32(2), u32(0), u32(0), None, out, None)
    add("cob_search_batch: null out", "plo_cob_search_batch", u32(1), u32(2), u32(2), u32(0), u32(0), prob4, None, None)
    add("cob_search_batch: the fourth problem's modulus", "plo_cob_search_batch", u32(4), u32(2), u32(2), u32(0), u32(0), prob4, out, None)
    add("cob_search_batch: bad dimensions", "plo_cob_search_batch", u32(1), u32(2), u32(2), u32(2), u32(0), prob4, out, None)
    # ---- trilplacer and inplacer: the device comes first
    add("tril_plan_create: null A", "plo_tril_plan_create", None, ref(I), ref(I), ref(h))
    add("tril_plan_create_x: null plan", "plo_tril_plan_create_x", ref(I), ref(I), ref(I), i32(0), None)
    add("tril_plan_create_x: null rowptr", "plo_tril_plan_create_x", ref(I), ref(Inull), ref(I), i32(0), ref(h))
    add("tril_plan_create_x: no plo_init", "plo_tril_plan_create_x", ref(I), ref(I), ref(I), i32(1), ref(h))
    add("tril_plan_create_q: no plo_init comes before null", "plo_tril_plan_create_q", None, None, None, i32(0), None)
    add("tril_plan_create_q: no plo_init", "plo_tril_plan_create_q", ref(Q), ref(Q), ref(Q), i32(0), ref(h))
    add("tril_plan_destroy: null", "plo_tril_plan_destroy", None)
    add("tril_cost_many: no plo_init comes before null", "plo_tril_cost_many", None, None, u64(0), u64(1), None, None)
    add("tril_cost_many: no plo_init comes before 2^31", "plo_tril_cost_many", fake, None, u64(0), u64(1 << 31), words, None)
    add("tril_search: no plo_init comes before null", "plo_tril_search", None, u64(0), u64(1), None, None)
    add("tril_search: no plo_init comes before the count", "plo_tril_search", fake, u64(0), u64(0), out, None)
    add("lin_plan_create_q: no plo_init comes before null", "plo_lin_plan_create_q", None, None)
    add("lin_plan_create_q: no plo_init", "plo_lin_plan_create_q", ref(Q), ref(h))
    add("lin_plan_destroy: null", "plo_lin_plan_destroy", None)
    add("lin_cost_many: no plo_init", "plo_lin_cost_many", fake, None, u64(0), u64(1), words, None)
    add("lin_search: no plo_init", "plo_lin_search", fake, u64(0), u64(1 << 31), out, None)
    # ---- orbiter
    add("orbit_plan_create_q: CSE measure", "plo_orbit_plan_create_q", ref(Q), ref(Q), ref(Q), u64(0), i32(1), ref(h))
    add("orbit_plan_create_q: growth measure", "plo_orbit_plan_create_q", ref(Q), ref(Q), ref(Q), u64(0), i32(3), ref(h))
    add("orbit_plan_create_act: growth measure and null", "plo_orbit_plan_create_act", None, ref(Q), ref(Q), u64(0), i32(3), i32(0), ref(h))
    add("orbit_plan_create_act: CSE measure comes before null", "plo_orbit_plan_create_act", None, None, None, u64(0), i32(1), i32(0), None)
    add("orbit_plan_create_act: null plan", "plo_orbit_plan_create_act", ref(Q), ref(Q), ref(Q), u64(0), i32(0), i32(0), None)
    add("orbit_plan_create_act: measure 7", "plo_orbit_plan_create_act", ref(Q), ref(Q), ref(Q), u64(0), i32(7), i32(0), ref(h))
    add("orbit_plan_create_act: no plo_init comes before the action and modulus 1", "plo_orbit_plan_create_act", ref(Q), ref(Q), ref(Q), u64(1), i32(2), i32(9), ref(h))
    add("orbit_plan_create_q: no plo_init", "plo_orbit_plan_create_q", ref(Q), ref(Q), ref(Q), u64(0), i32(0), ref(h))
    add("orbit_plan_create_cse: null R", "plo_orbit_plan_create_cse", ref(Q), None, ref(Q), u64(7), i32(0), u32(1), u64(0), ref(h))
    for mod in (0, 1, 8, 9, 1 << 31, (1 << 31) + 11):
        add("orbit_plan_create_cse: modulus %d" % mod, "plo_orbit_plan_create_cse", ref(Q), ref(Q), ref(Q), u64(mod), i32(0), u32(1), u64(0), ref(h))
    add("orbit_plan_create_cse: sub 0", "plo_orbit_plan_create_cse", ref(Q), ref(Q), ref(Q), u64(7), i32(0), u32(0), u64(0), ref(h))
    add("orbit_plan_create_cse: sub 65537", "plo_orbit_plan_create_cse", ref(Q), ref(Q), ref(Q), u64(7), i32(0), u32(65537), u64(0), ref(h))
    add("orbit_plan_create_cse: no plo_init", "plo_orbit_plan_create_cse", ref(Q), ref(Q), ref(Q), u64(2147483629), i32(0), u32(65536), u64(0), ref(h))
    add("orbit_plan_create_growth: null plan", "plo_orbit_plan_create_growth", ref(Q), ref(Q), ref(Q), i32(0), None)
    add("orbit_plan_create_growth: Householder", "plo_orbit_plan_create_growth", ref(Q), ref(Q), ref(Q), i32(2), ref(h))
    add("orbit_plan_create_growth: no plo_init", "plo_orbit_plan_create_growth", ref(Q), ref(Q), ref(Q), i32(1), ref(h))
    add("orbit_plan_info: null plan", "plo_orbit_plan_info", None, words)
    add("orbit_plan_info: null out", "plo_orbit_plan_info", fake, None)
    add("orbit_plan_destroy: null", "plo_orbit_plan_destroy", None)
    add("orbit_cost_many: no plo_init comes before null", "plo_orbit_cost_many", None, None, u64(0), u64(1), words, None)
    add("orbit_cost_many: no plo_init", "plo_orbit_cost_many", fake, None, u64(0), u64(1), words, None)
    add("orbit_search: no plo_init comes before null", "plo_orbit_search", None, u64(0), u64(1), out, None)
    add("orbit_search: no plo_init", "plo_orbit_search", fake, u64(0), u64(0), out, None)
    add("orbit_growth_many: null cost", "plo_orbit_growth_many", fake, None, u64(0), u64(1), None, words, None)
    add("orbit_growth_many: no growth plan", "plo_orbit_growth_many", fake, None, u64(0), u64(1), dbl, words, None)
    add("orbit_growth_search: no plo_init comes before null", "plo_orbit_growth_search", None, u64(0), u64(1), out, None)
    add("orbit_growth_search: no plo_init", "plo_orbit_growth_search", fake, u64(0), u64(1), out, None)
    # ---- dependency
    add("dep_plan_create_q: no plo_init comes before null", "plo_dep_plan_create_q", None, None, None, u32(1), u64(0), u32(2), None)
    add("dep_plan_create_q: no plo_init", "plo_dep_plan_create_q", ref(Q), (ctypes.c_int64 * 1)(1), (ctypes.c_int64 * 1)(1), u32(1), u64(1), u32(0), ref(h))
    add("dep_plan_destroy: null", "plo_dep_plan_destroy", None)
    add("dep_search: no plo_init comes before null", "plo_dep_search", None, u32(0), u32(1), None, u64(0), None, None)
    add("dep_search: no plo_init", "plo_dep_search", fake, u32(1), u32(0), None, u64(0), w64, None)
    labels = [t[0] for t in T]
    for k, t in enumerate(T):                                        # the change-of-basis rows share a label: number them
        if labels.count(t[0]) > 1:
            T[k] = ("%s #%d" % (t[0], labels[:k].count(t[0]) + 1),) + t[1:]
    return T


def child():
    L = ctypes.CDLL(LIB)
    L.plo_last_error.restype = ctypes.c_char_p
    L.plo_pack_cost.restype = L.plo_multi_comm_inits.restype = ctypes.c_uint64
    for name in ("plo_tril_plan_destroy", "plo_lin_plan_destroy", "plo_orbit_plan_destroy", "plo_dep_plan_destroy"):
        getattr(L, name).restype = None
    rows = [{"call": "plo_last_error before any call", "rc": None, "error": L.plo_last_error().decode()}]
    for label, fn, args in calls(L):
        rc = fn(*args)
        failed = fn.restype is not None and fn.restype is not ctypes.c_uint64 and rc < 0
        rows.append({"call": label, "rc": rc, "error": L.plo_last_error().decode() if failed else None})
    json.dump(rows, sys.stdout, indent=0)


def run_child():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_refusals_match_the_recorded_ones():
    got = run_child()
    want = json.load(open(GOLDEN))
    assert [g["call"] for g in got] == [w["call"] for w in want]
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, "\n".join("%s: got (%s, %r), recorded (%s, %r)" % (g["call"], g["rc"], g["error"], w["rc"], w["error"]) for g, w in bad)
    # the missing-plo_init refusal is in the table in both wordings that need no device (the third is plo_init's own)
    texts = {w["error"] for w in want}
    assert {"plo_init not called", "plo_init was not called (or found no HIP device)"} <= texts


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    elif "--record" in sys.argv:
        rows = run_child()
        with open(GOLDEN, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
        print("%d calls recorded from %s" % (len(rows), LIB))
