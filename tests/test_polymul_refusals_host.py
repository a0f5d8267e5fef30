"""What the plo_polymul_* entries answer before they look for a device: the code and the text of every refusal that
include/plinopt_hip.h names for them, through plinopt_amd.capi.  The argument checks come first, the missing plo_init after
them.  One child process makes the calls: it never calls plo_init, so it answers the same with and without a GPU.  Where an
entry takes a plan, a zeroed buffer stands for one: a plan of no pairs, which is all these refusals read."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_HIP, E_CAPACITY = -1, -2, -3

# (label, expected code, a piece of the expected text)
WANT = [
    ("null L", E_ARG, "null argument"), ("null R", E_ARG, "null argument"), ("null P", E_ARG, "null argument"), ("null plan", E_ARG, "null argument"),
    ("null fnum with flen 3", E_ARG, "null argument"),
    ("L.m != R.m", E_ARG, "inner dimensions 7, 8, 7 of L, R and P differ"), ("L.m != P.n", E_ARG, "inner dimensions 7, 7, 8 of L, R and P differ"),
    ("q = 0", E_ARG, "modulus 0 outside 2 .. 2^31 - 1"), ("q = 1", E_ARG, "modulus 1 outside"), ("q = 2^31", E_ARG, "modulus 2147483648 outside"),
    ("unsorted row", E_ARG, "columns must be sorted and in range"), ("column out of range", E_ARG, "columns must be sorted and in range"),
    ("zero entry", E_ARG, "zero entry or non-positive denominator"), ("negative denominator", E_ARG, "zero entry or non-positive denominator"),
    ("row pointers decrease", E_ARG, "row pointers decrease"), ("null arrays", E_ARG, "null arrays"),
    ("flen = 1", E_ARG, "a constant polynomial"), ("leading coefficient 0", E_ARG, "the leading coefficient of the polynomial is 0"),
    ("fden = 0", E_ARG, "a non-positive denominator in the polynomial"),
    ("denominator 3 modulo 3", E_ARG, "a denominator is no unit modulo 3"), ("denominator 6 modulo 15", E_ARG, "a denominator is no unit modulo 15"),
    ("denominator of f", E_ARG, "a denominator of the polynomial is no unit modulo 3"),
    ("leading coefficient 3 modulo 3", E_ARG, "the leading coefficient of the polynomial is no unit modulo 3"),
    ("leading coefficient 2 modulo 6", E_ARG, "the leading coefficient of the polynomial is no unit modulo 6"),
    ("na above 16384", E_CAPACITY, "more than 16384 columns in L or R"), ("nb above 16384", E_CAPACITY, "more than 16384 columns in L or R"),
    ("Z above 32768 by nc", E_CAPACITY, "max(nc, na + nb - 1) above 32768"), ("rank above 2^20", E_CAPACITY, "rank above 2^20"),
    ("fold of degree 2049", E_CAPACITY, "a fold modulo a polynomial of degree above 2048"),
    ("no plo_init", E_HIP, "plo_init was not called"),
    ("no plo_init with a polynomial", E_HIP, "plo_init was not called"),
    ("composite modulus with a unit leading coefficient gets to the device check", E_HIP, "plo_init was not called"),
    ("fold of degree 2048 gets to the device check", E_HIP, "plo_init was not called"),
    ("degree 2049 above Z (no fold) gets to the device check", E_HIP, "plo_init was not called"),
    ("na = nb = 16384 gets to the device check", E_HIP, "plo_init was not called"),
    ("check: null plan", E_ARG, "null argument"), ("check: null result", E_ARG, "null argument"),
    ("check: empty range", E_ARG, "pairs 3 .. 3: an empty range or one beyond the 0 pairs"), ("check: range beyond the pairs", E_ARG, "pairs 0 .. 1: an empty range or one beyond"),
    ("info: null plan", E_ARG, "null argument"), ("info: null out", E_ARG, "null argument"),
    ("destroy: null", None, None),
]


def child():
    sys.path.insert(0, ROOT)
    from plinopt_amd import capi
    L = capi.lib()
    ref = ctypes.byref

    def q(m, n, rowptr, col, num, den=None, null=False):
        rp = (ctypes.c_uint32 * len(rowptr))(*rowptr)
        c = (ctypes.c_uint32 * max(len(col), 1))(*col)
        nu = (ctypes.c_int64 * max(len(num), 1))(*num)
        de = (ctypes.c_int64 * max(len(num), 1))(*(den or [1] * len(num)))
        if null:
            return capi.QCSR(m, n, rp, None, None, None)
        return capi.QCSR(m, n, rp, c, nu, de)

    def mat(m, n, **kw):                                                          # one entry 1 in row 0, column 0
        return q(m, n, [0] + [1] * m, [0], [1], **kw)

    def empty(m, n):
        return q(m, n, [0] * (m + 1), [], [])

    h = ctypes.c_void_p()
    Lm, Rm, Pm = mat(7, 3), mat(7, 3), mat(5, 7)
    rows = []

    def create(label, A=Lm, B=Rm, C=Pm, f=(), fden=None, mod=7, plan=True, fnull=False):
        fn = (ctypes.c_int64 * max(len(f), 1))(*f)
        fd = (ctypes.c_int64 * max(len(f), 1))(*(fden or [1] * len(f)))
        rc = L.plo_polymul_plan_create_q(ref(A) if A is not None else None, ref(B) if B is not None else None, ref(C) if C is not None else None,
                                         None if fnull else fn, None if fnull else fd, 3 if fnull else len(f), mod, ref(h) if plan else None)
        rows.append((label, rc, L.plo_last_error().decode() if rc else None))

    create("null L", A=None); create("null R", B=None); create("null P", C=None); create("null plan", plan=False)
    create("null fnum with flen 3", fnull=True)
    create("L.m != R.m", B=mat(8, 3)); create("L.m != P.n", C=mat(5, 8))
    create("q = 0", mod=0); create("q = 1", mod=1); create("q = 2^31", mod=1 << 31)
    create("unsorted row", A=q(7, 3, [0, 2] + [2] * 6, [1, 0], [1, 1]))
    create("column out of range", B=q(7, 3, [0, 1] + [1] * 6, [3], [1]))
    create("zero entry", C=q(5, 7, [0, 1, 1, 1, 1, 1], [0], [0]))
    create("negative denominator", A=q(7, 3, [0, 1] + [1] * 6, [0], [1], [-2]))
    create("row pointers decrease", A=q(7, 3, [0, 2, 1] + [2] * 5, [0, 1], [1, 1]))
    create("null arrays", A=mat(7, 3, null=True))
    create("flen = 1", f=[5]); create("leading coefficient 0", f=[1, 1, 0])
    create("fden = 0", f=[1, 1, 1], fden=[1, 0, 1])
    create("denominator 3 modulo 3", A=q(7, 3, [0, 1] + [1] * 6, [0], [1], [3]), mod=3)
    create("denominator 6 modulo 15", C=q(5, 7, [0, 1, 1, 1, 1, 1], [0], [5], [6]), mod=15)
    create("denominator of f", f=[1, 1, 1], fden=[3, 1, 1], mod=3)
    create("leading coefficient 3 modulo 3", f=[1, 1, 3], mod=3)
    create("leading coefficient 2 modulo 6", f=[1, 1, 2], mod=6)
    create("na above 16384", A=mat(1, 16385), B=mat(1, 1), C=mat(1, 1)); create("nb above 16384", A=mat(1, 1), B=mat(1, 16385), C=mat(1, 1))
    create("Z above 32768 by nc", A=mat(1, 1), B=mat(1, 1), C=empty(32769, 1))
    big = (1 << 20) + 1
    create("rank above 2^20", A=empty(big, 1), B=empty(big, 1), C=empty(1, big))
    wide = (mat(1, 2000), mat(1, 2000), mat(1, 1))                                 # Z = 3999
    create("fold of degree 2049", *wide, f=[1] * 2050)
    create("no plo_init")
    create("no plo_init with a polynomial", f=[1, -1, 0, 0, 0, 1], mod=3)
    create("composite modulus with a unit leading coefficient gets to the device check", f=[2, 3, 5], mod=6)
    create("fold of degree 2048 gets to the device check", *wide, f=[1] * 2049)
    create("degree 2049 above Z (no fold) gets to the device check", f=[1] * 2050)
    create("na = nb = 16384 gets to the device check", A=mat(1, 16384), B=mat(1, 16384), C=mat(1, 1))
    fake = ctypes.create_string_buffer(1 << 16)                     # as in test_brent_refusals_host.py: a plan read as zeros (no pairs, no device memory); never launched
    res, out = capi.BrentResult(), (ctypes.c_uint32 * 8)()
    for label, fn, args in (("check: null plan", L.plo_polymul_check, (None, 0, 1, ref(res), None)), ("check: null result", L.plo_polymul_check, (fake, 0, 1, None, None)),
                            ("check: empty range", L.plo_polymul_check, (fake, 3, 3, ref(res), None)), ("check: range beyond the pairs", L.plo_polymul_check, (fake, 0, 1, ref(res), None)),
                            ("info: null plan", L.plo_polymul_plan_info, (None, out)), ("info: null out", L.plo_polymul_plan_info, (fake, None))):
        rc = fn(*args)
        rows.append((label, rc, L.plo_last_error().decode() if rc else None))
    L.plo_polymul_plan_destroy(None)
    rows.append(("destroy: null", None, None))
    json.dump(rows, sys.stdout)


def test_refusals_have_their_codes_and_texts():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    assert [g[0] for g in got] == [w[0] for w in WANT]
    for (label, rc, text), (_, wrc, wtext) in zip(got, WANT):
        assert rc == wrc, (label, rc, text)
        if wtext is not None:
            assert wtext in text, (label, text)


def test_python_mirror_is_exported():
    import plinopt_amd
    assert callable(plinopt_amd.PolyMulPlan)
    for s in ("plo_polymul_plan_create_q", "plo_polymul_check", "plo_polymul_plan_info", "plo_polymul_plan_destroy"):
        assert s in plinopt_amd.capi.EXPORTS


def test_the_header_states_the_fold_limit():
    text = open(os.path.join(ROOT, "include", "plinopt_hip.h")).read()
    assert "#define PLO_POLYMUL_MAX_FOLD_DEGREE 2048u" in text


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
