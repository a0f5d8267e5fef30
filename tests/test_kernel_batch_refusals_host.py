"""What plo_kernel_batch_search answers before it looks for a device: PLO_E_ARG and a text for every argument the header
names.  No plo_init, no GPU."""
import ctypes

import pytest


def _call(nprob=1, mats=True, p=131071, per=3, mode=0, bests=True, status=True, csr=(2, 2, [0, 2, 4], [0, 1, 0, 1], [1, 1, 1, 1])):
    from plinopt_amd import capi
    L = capi.lib()
    c, keep = capi.make_csr(*csr)
    A = (capi.CSR * 1)(c)
    b, s, st = (capi.Best * 1)(), (ctypes.c_int32 * 1)(), capi.Stats()
    rc = L.plo_kernel_batch_search(nprob, A if mats else None, p, 0, per, mode, b if bests else None, s if status else None, ctypes.byref(st))
    del keep
    return rc, L.plo_last_error().decode()


@pytest.mark.parametrize("what,kw", [
    ("null mats", dict(mats=False)), ("null bests", dict(bests=False)), ("null status", dict(status=False)),
    ("no problem", dict(nprob=0)), ("no restart", dict(per=0)),
    ("even modulus", dict(p=131072)), ("modulus 1", dict(p=1)), ("modulus 2^31", dict(p=2 ** 31)), ("modulus 2^31 + 11", dict(p=2 ** 31 + 11)),
    ("cost mode -1", dict(mode=-1)), ("cost mode 3", dict(mode=3)),
    ("2^32 candidates", dict(nprob=2 ** 16, per=2 ** 16)),
    ("column beyond n", dict(csr=(2, 2, [0, 2, 4], [0, 2, 0, 1], [1, 1, 1, 1]))),
    ("zero value", dict(csr=(2, 2, [0, 2, 4], [0, 1, 0, 1], [1, 0, 1, 1]))),
    ("row pointers not increasing", dict(csr=(2, 2, [0, 3, 2], [0, 1, 0, 1], [1, 1, 1, 1]))),
])
def test_argument_refusals(what, kw):
    from plinopt_amd import capi
    rc, msg = _call(**kw)
    assert rc == capi.PLO_E_ARG and msg, (what, rc, msg)


def test_python_mirror_is_exported():
    import plinopt_amd
    assert callable(plinopt_amd.kernel_batch_search) and "plo_kernel_batch_search" in plinopt_amd.capi.EXPORTS
