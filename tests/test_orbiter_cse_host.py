"""bin/orbiter -z on the host (--gpu 0): the CSE measure (PLO_ORBIT_CSE, include/plinopt_hip.h) held to the literal oracle
tests/orbit_cse_oracle.py -- per-seed lines of --costs, the winner of a search, the files it writes and --candidate -- and the
refusals of the tool and of the C API."""
import ctypes
import os
import shutil
import subprocess

import pytest

import orbit_action_oracle as A
import orbit_cse_oracle as Z
import orbit_oracle as O
import synth
from plo_testlib import DATA, ROOT, read_sms

ORB = os.path.join(ROOT, "bin", "orbiter")


def run(cmd, timeout=300):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout, r.stderr


def files(name, d=DATA):
    return [os.path.join(d, "%s_%s.sms" % (name, x)) for x in "LRP"]


def default_sub(loops):
    return loops >> 4 if loops > 16 else 1                                     # reference src/orbiter.cpp:257


@pytest.mark.parametrize("name,n,sub,p,action", [
    ("2x2x2_7_Winograd", 64, 1, 131071, "triangular"), ("2x2x2_7_Winograd", 64, 3, 131071, "triangular"),
    ("2x2x2_7_Strassen", 16, None, 131071, "triangular"), ("2x2x2_7_Strassen", 16, None, 131071, "pluq"), ("2x2x2_7_Strassen", 16, None, 131071, "householder"),
    ("3x3x3_23_58", 8, 2, 131071, "triangular"),
    ("2x2x2_7_Winograd", 64, None, 3, "triangular"), ("2x2x2_7_Winograd", 64, None, 2147483629, "triangular")])
def test_costs_equal_the_oracle_line_by_line(name, n, sub, p, action):
    """fails without the feature: the parent ignores -z modulo a number and prints density counts"""
    cmd = [ORB, "--gpu", "0", "-q", str(p), "-z", "--costs", "-O", str(n), "--action", action] + (["--sub", str(sub)] if sub else []) + files(name)
    rc, out, err = run(cmd)
    assert rc == 0, err
    got = [tuple(map(int, ln.split())) for ln in out.splitlines()]
    mats, mkn = O.load(os.path.join(DATA, name))
    want, _ = Z.costs(mats, mkn, [O.BASE_SEED] + list(range(n)), p, sub or default_sub(n), 0, A.ACTIONS[action])
    assert got == want, next((j, a, b) for j, (a, b) in enumerate(zip(got, want)) if a != b)
    assert any(c != z for c, z, _ in want)                                     # the measure is not the density count


def test_search_winner_files_and_candidate(tmp_path):
    name, p, n = "2x2x2_7_Strassen", 131071, 40
    for f in files(name):
        shutil.copy(f, tmp_path)
    src = files(name, str(tmp_path))
    rc, out, err = run([ORB, "--gpu", "0", "-q", str(p), "-z", "-O", str(n)] + src)
    assert rc == 0, err
    mats, mkn = O.load(os.path.join(DATA, name))
    sub = default_sub(n)
    per, best = Z.costs(mats, mkn, list(range(n)), p, sub, 0)
    init = Z.cost3(mats, mkn, O.BASE_SEED, p, sub, 0)
    assert best[:3] < init                                                     # (the search improves on the input: files are written)
    assert out.split() == ["winner"] + [str(x) for x in best]
    assert "# Init. ops: %d, (%d,%d)" % init in err and "Rdcd. opt: %d<%d" % (best[0], init[0]) in err
    assert "%d Optimizer runs" % (n * 3 * sub) in err.splitlines()[-1] and "restarts on host" in err.splitlines()[-1]
    written = [p_[:-4] + ".nnz.sms" for p_ in src]
    got = [O.dense(*read_sms(f)) for f in written]
    assert O.mm_check(*got, mkn, modulus=p)
    assert O.counts(*got, modulus=p)[1:] == best[1:3]
    d = tmp_path / "cand"
    rc, _, err = run([ORB, "--gpu", "0", "-q", str(p), "-z", "-O", str(n), "--candidate", str(best[3]), str(d)] + src)
    assert rc == 0, err
    assert "candidate %d: %d %d %d" % (best[3], best[0], best[1], best[2]) in err
    for w, x in zip(written, "LRP"):
        assert open(w, "rb").read() == open(str(d / (x + ".sms")), "rb").read()


@pytest.mark.parametrize("args", [["-z", "-q", "15"], ["-z"], ["-z", "-q", "131071", "--sub", "0"]])
def test_refusals_exit_2(args):
    rc, out, err = run([ORB, "--gpu", "0", "-O", "5"] + args + files("2x2x2_7_Strassen"))
    assert rc == 2, (rc, err)
    assert "ERROR" in err and not out


def test_prime_of_2_31_or_more_runs_on_the_host_and_says_so(tmp_path):
    """(the CPU oracle keeps 31-bit residues: here the counts nnz and nno are checked, and that the cost is below them)"""
    p, src = 2147483659, files("2x2x2_7_Winograd")
    rc, out, err = run([ORB, "--gpu", "0", "-q", str(p), "-z", "--costs", "-O", "4"] + src)
    assert rc == 0, err
    mats, mkn = O.load(os.path.join(DATA, "2x2x2_7_Winograd"))
    got = [tuple(map(int, ln.split())) for ln in out.splitlines()]
    assert [g[1:] for g in got] == [O.cost3(mats, mkn, s, modulus=p)[1:] for s in [O.BASE_SEED] + list(range(4))]
    assert all(0 < g[0] < g[1] for g in got)
    for f in src:
        shutil.copy(f, tmp_path)
    rc, out, err = run([ORB, "--gpu", "1", "-q", str(p), "-z", "-O", "4"] + files("2x2x2_7_Winograd", str(tmp_path)))      # refused before the library is loaded
    assert rc == 0, err
    assert "host search" in err and "restarts on host" in err
    best = min(g + (s,) for g, s in zip(got[1:], range(4)))
    assert out.split() == ["winner"] + ([str(x) for x in best] if best[:3] < got[0] else [str(x) for x in got[0]] + ["base"])


def test_c_api_refusals():
    from plinopt_amd import capi
    L = capi.lib()
    csr = [synth.qcsr(*read_sms(f)) for f in files("2x2x2_7_Winograd")]
    from plinopt_amd.search import _qcsr
    held = [_qcsr(*(tuple(M) + (None,) * (6 - len(M)))) for M in csr]
    a = [ctypes.byref(c) for c, _ in held]
    h = ctypes.c_void_p()
    # the create functions of the other measures carry no sub: measure 1 is an argument error, device or not
    assert L.plo_orbit_plan_create_act(*a, 131071, 1, 0, ctypes.byref(h)) == capi.PLO_E_ARG
    assert L.plo_orbit_plan_create_q(*a, 131071, 1, ctypes.byref(h)) == capi.PLO_E_ARG
    for bad_mod in (0, 4, 15, 1 << 31, 2147483659):
        assert L.plo_orbit_plan_create_cse(*a, bad_mod, 0, 1, 0, ctypes.byref(h)) == capi.PLO_E_ARG, bad_mod
    assert L.plo_orbit_plan_create_cse(*a, 131071, 0, 0, 0, ctypes.byref(h)) == capi.PLO_E_ARG      # sub 0
    assert L.plo_orbit_plan_info(None, (ctypes.c_uint32 * 8)()) == capi.PLO_E_ARG


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from plinopt_amd import ORBIT_CSE, OrbitPlan, capi
    csr = [synth.qcsr(*read_sms(f)) for f in files("2x2x2_7_Winograd")]
    with pytest.raises(capi.PloError) as e:
        OrbitPlan(*csr, modulus=131071, measure=ORBIT_CSE, sub=2)
    assert e.value.code == capi.PLO_E_HIP
