"""What the plo_brent_* entries answer before they look for a device: the code and the text of every refusal that
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
    ("null L", E_ARG, "null argument"), ("null P", E_ARG, "null argument"), ("null plan", E_ARG, "null argument"),
    ("m = 0", E_ARG, "m, k and n must be positive"),
    ("L.n != mk", E_ARG, "7x5, 7x4, 4x7 are not r x mk, r x kn, mn x r for 2x2x2"),
    ("R.n != kn", E_ARG, "are not r x mk, r x kn, mn x r"), ("P.m != mn", E_ARG, "are not r x mk, r x kn, mn x r"),
    ("L.m != R.m", E_ARG, "are not r x mk, r x kn, mn x r"), ("L.m != P.n", E_ARG, "are not r x mk, r x kn, mn x r"),
    ("q = 0", E_ARG, "modulus 0 outside 2 .. 2^31 - 1"), ("q = 1", E_ARG, "modulus 1 outside"), ("q = 2^31", E_ARG, "modulus 2147483648 outside"),
    ("unsorted row", E_ARG, "columns must be sorted and in range"), ("column out of range", E_ARG, "columns must be sorted and in range"),
    ("zero entry", E_ARG, "zero entry or non-positive denominator"), ("negative denominator", E_ARG, "zero entry or non-positive denominator"),
    ("row pointers decrease", E_ARG, "row pointers decrease"), ("null arrays", E_ARG, "null arrays"),
    ("denominator 3 modulo 3", E_ARG, "a denominator is no unit modulo 3"), ("denominator 6 modulo 15", E_ARG, "a denominator is no unit modulo 15"),
    ("mk above 16384", E_CAPACITY, "mk, kn or mn above 16384"), ("rank above 2^20", E_CAPACITY, "rank above 2^20"),
    ("no plo_init", E_HIP, "plo_init was not called"),
    ("composite modulus gets to the device check", E_HIP, "plo_init was not called"),
    ("32x32x32 of rank 15096 gets to the device check", E_HIP, "plo_init was not called"),
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

    h = ctypes.c_void_p()
    Lm, Rm, Pm = mat(7, 4), mat(7, 4), mat(4, 7)
    rows = []

    def create(label, A=Lm, B=Rm, C=Pm, mkn=(2, 2, 2), mod=7, plan=True):
        rc = L.plo_brent_plan_create_q(ref(A) if A is not None else None, ref(B) if B is not None else None, ref(C) if C is not None else None,
                                       mkn[0], mkn[1], mkn[2], mod, ref(h) if plan else None)
        rows.append((label, rc, L.plo_last_error().decode() if rc else None))

    create("null L", A=None); create("null P", C=None); create("null plan", plan=False)
    create("m = 0", mkn=(0, 2, 2))
    create("L.n != mk", A=mat(7, 5)); create("R.n != kn", B=mat(7, 6)); create("P.m != mn", C=mat(5, 7))
    create("L.m != R.m", B=mat(8, 4)); create("L.m != P.n", C=mat(4, 8))
    create("q = 0", mod=0); create("q = 1", mod=1); create("q = 2^31", mod=1 << 31)
    create("unsorted row", A=q(7, 4, [0, 2] + [2] * 6, [1, 0], [1, 1]))
    create("column out of range", B=q(7, 4, [0, 1] + [1] * 6, [4], [1]))
    create("zero entry", C=q(4, 7, [0, 1, 1, 1, 1], [0], [0]))
    create("negative denominator", A=q(7, 4, [0, 1] + [1] * 6, [0], [1], [-2]))
    create("row pointers decrease", A=q(7, 4, [0, 2, 1] + [2] * 5, [0, 1], [1, 1]))
    create("null arrays", A=mat(7, 4, null=True))
    create("denominator 3 modulo 3", A=q(7, 4, [0, 1] + [1] * 6, [0], [1], [3]), mod=3)
    create("denominator 6 modulo 15", C=q(4, 7, [0, 1, 1, 1, 1], [0], [5], [6]), mod=15)
    create("mk above 16384", A=mat(1, 16385), B=mat(1, 1), C=mat(16385, 1), mkn=(16385, 1, 1))
    big = (1 << 20) + 1
    create("rank above 2^20", A=q(big, 1, [0] * (big + 1), [], []), B=q(big, 1, [0] * (big + 1), [], []), C=q(1, big, [0, 0], [], []), mkn=(1, 1, 1))
    create("no plo_init")
    create("composite modulus gets to the device check", mod=2147483629 - 2)
    r = 15096
    create("32x32x32 of rank 15096 gets to the device check", A=q(r, 1024, [0] * (r + 1), [], []), B=q(r, 1024, [0] * (r + 1), [], []), C=q(1024, r, [0] * 1025, [], []), mkn=(32, 32, 32), mod=2147483629)
    fake = ctypes.create_string_buffer(1 << 16)                     # as in test_capi_refusals_host.py: a plan read as zeros (no pairs, no device memory); never launched
    res, out = capi.BrentResult(), (ctypes.c_uint32 * 8)()
    for label, fn, args in (("check: null plan", L.plo_brent_check, (None, 0, 1, ref(res), None)), ("check: null result", L.plo_brent_check, (fake, 0, 1, None, None)),
                            ("check: empty range", L.plo_brent_check, (fake, 3, 3, ref(res), None)), ("check: range beyond the pairs", L.plo_brent_check, (fake, 0, 1, ref(res), None)),
                            ("info: null plan", L.plo_brent_plan_info, (None, out)), ("info: null out", L.plo_brent_plan_info, (fake, None))):
        rc = fn(*args)
        rows.append((label, rc, L.plo_last_error().decode() if rc else None))
    L.plo_brent_plan_destroy(None)
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
    assert callable(plinopt_amd.BrentPlan)
    for s in ("plo_brent_plan_create_q", "plo_brent_check", "plo_brent_plan_info", "plo_brent_plan_destroy"):
        assert s in plinopt_amd.capi.EXPORTS


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
