"""`bin/optimizer -N` by order index on the host (`--gpu 0`: the walk of 10 to 12 rows and of `--orders` ranges, OpenMP over
the order indices) against the oracle's prescribed-order decomposition; the usage errors of `--orders`; what
`plo_kernel_search_orders` answers before it touches a device."""
import itertools
import math
import os
import re
import subprocess
import sys

import pytest

from kernel_orders_lib import P, fixture, kth_permutation, oracle_best, oracle_range
from plo_testlib import DATA, ROOT

OPT = os.path.join(ROOT, "bin", "optimizer")
CHK = os.path.join(ROOT, "bin", "SLPchecker")
F = math.factorial
N_PAT = r"# Found N: (\d+)\|(\d+) instead of \d+\|\d+\t\[order (\d+), seed (\d+)\] \((\d+) of (\d+) row orders from (\d+), (\d+) restarts each, host\)"


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "plinopt_amd", "csrc", "host")])


def run(cmd, stdin=None):
    r = subprocess.run(cmd, input=stdin, capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def test_kth_permutation_is_the_lexicographic_order():
    assert [tuple(kth_permutation(4, k)) for k in range(24)] == list(itertools.permutations(range(4)))


@pytest.mark.parametrize("name,first,count,loops", [
    ("4o4o4_S243_10-43_L", 1814144, 2000, 100),             # 5 * 9! - 256; -O below 10!: one restart per order
    ("4o4o4_F243-11-44_L", 7 * F(10) - 100, 400, 2 * F(11)),      # 11 rows, a carry in the leading digit, two restarts per order
])
def test_host_walk_of_a_range_equals_the_oracle(name, first, count, loops):
    path = os.path.join(DATA, name + ".sms")
    M = fixture(name)
    sub = max(1, loops // F(M.m))
    rc, out, err = run([OPT, "-q", str(P), "--only", "N", "--orders", "%d:%d" % (first, count), "--seed", "11", "-O", str(loops), "--gpu", "0", path])
    assert rc == 0 and "-N skipped" not in err, err
    g = re.search(N_PAT, err)
    assert g, err
    a, mu, seed = oracle_best(oracle_range(M, 11, first, count, sub), 11, first, sub)
    assert tuple(int(x) for x in g.groups()) == (a, mu, (seed - 11) // sub, seed, count, F(M.m), first, sub)
    rc, _, err2 = run([CHK, "-q", str(P), "-M", path], stdin=out)
    assert rc == 0 and "SUCCESS" in err2, err2


def test_orders_selects_the_walk_by_index_below_ten_rows():
    """--orders on 7 rows: the no-dedup walk over all 5040 orders by index, against the oracle"""
    name = "2x2x2_7_Winograd_L"
    M = fixture(name)
    rc, out, err = run([OPT, "-q", str(P), "--only", "N", "--orders", "0:5040", "--seed", "3", "--gpu", "0", os.path.join(DATA, name + ".sms")])
    assert rc == 0, err
    g = re.search(N_PAT, err)
    a, mu, seed = oracle_best(oracle_range(M, 3, 0, 5040, 1), 3, 0, 1)
    assert g and tuple(int(x) for x in g.groups()) == (a, mu, seed - 3, seed, 5040, 5040, 0, 1), err


@pytest.mark.parametrize("args,what", [
    (["-D", "--orders", "0:10"], "--orders is a range of the row orders of -N"),                       # without -N
    (["--only", "N", "--orders", "%d:2" % (F(10) - 1)], "is no range of the 3628800 orders"),          # past 10!
    (["--only", "N", "--orders", "0:0"], "is no range of the 3628800 orders"),
    (["--only", "N", "--orders", "12"], "--orders takes first:count"),
])
def test_orders_usage_errors(args, what):
    rc, out, err = run([OPT, "-q", str(P), "--gpu", "0"] + args + [os.path.join(DATA, "4o4o4_S243_10-43_L.sms")])
    assert rc != 0 and out == "" and what in err, (rc, err)


def test_thirteen_rows_are_skipped():
    sms = "13 2 M\n" + "".join("%d 1 1\n" % (i + 1) for i in range(13)) + "0 0 0\n"
    rc, out, err = run([OPT, "-q", str(P), "--only", "N", "--gpu", "0"], stdin=sms)
    assert rc == 0 and "# -N skipped: 13 rows" in err, err


CHILD = r"""
import ctypes, sys
L = ctypes.CDLL(sys.argv[1])
L.plo_last_error.restype = ctypes.c_char_p
u32, u64 = ctypes.c_uint32, ctypes.c_uint64
class CSR(ctypes.Structure):
    _fields_ = [("m", u32), ("n", u32), ("rowptr", ctypes.POINTER(u32)), ("col", ctypes.POINTER(u32)), ("val", ctypes.POINTER(u32))]
def mat(m):
    return CSR(m, 1, (u32 * (m + 1))(*range(m + 1)), (u32 * m)(*([0] * m)), (u32 * m)(*([1] * m)))
out = ctypes.create_string_buffer(64)
def call(M, first, count, sub, mode=0):
    rc = L.plo_kernel_search_orders(ctypes.byref(M), u32(7), u64(0), u64(first), u64(count), u32(sub), ctypes.c_int(mode), None, None, None, out, None)
    print(rc, L.plo_last_error().decode())
call(mat(3), 0, 6, 1)        # nothing wrong with the arguments: no plo_init
call(mat(13), 0, 1, 1)
call(mat(1), 0, 1, 1)
call(mat(3), 0, 7, 1)        # first + count = 3! + 1
call(mat(3), 6, 1, 1)
call(mat(3), 0, 6, 0)
call(mat(3), 0, 0, 1)
call(mat(3), 0, 6, 1, 3)
"""


def test_entry_refuses_without_a_device():
    """the new entry before plo_init: PLO_E_HIP in the words of its siblings of the CSE family; its argument checks come first"""
    lib = os.environ.get("PLO_HIP_LIB") or os.path.join(ROOT, "plinopt_amd", "libplinopt_hip.so")
    r = subprocess.run([sys.executable, "-c", CHILD, lib], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "-2 plo_init not called"
    assert [ln.split()[0] for ln in lines[1:]] == ["-1"] * 7, lines
    assert "12 rows" in lines[1] and "beyond m!" in lines[3] and "beyond m!" in lines[4] and "cost mode" in lines[7]
