"""bin/TPchecker --gpu 0: the host loop held to the independent definition of tests/tprog_cases.py on every case and field, to
bin/trilplacer's own programs on the small fixture triples, and to its refusals and partial ranges.  No GPU."""
import glob
import os
import re
import subprocess

import pytest

import tprog_cases as C
from plo_testlib import DATA, ROOT, read_sms

TRILPLACER = os.path.join(ROOT, "bin", "trilplacer")
FIELDS = (0, 3, 15, 131071, C.P31, C.P62)
CASES = C.edge_cases("issue") + C.edge_cases("units") + [m for m, _ in C.mutations()] + [m for m, _ in C.mutations(C.schoolbook(3, 5, True, "units"))] + [C.hidden_defect()]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "plinopt_amd", "csrc", "host")])


def field(q):
    return "Z/%dZ" % q if q else "Q"


def held_to_definition(case, paths, q, gpu=0, env=None):
    """one case over one field: verdict, first equation, --count and exit status against the definition -> the --count text"""
    opts = case.flags() + (["-q", q] if q else [])
    try:
        want = C.definition(case, q)
    except C.Refused as r:
        rc, err = C.tool(opts + paths, gpu, env=env)
        assert rc == 4 and C.KINDS[r.kind] in err and "SUCCESS" not in err, err
        assert r.line is None or "line %d:" % r.line in err
        return err
    rc, err = C.tool(opts + ["--count"] + paths, gpu, env=env)
    if want[0] == 0:
        assert rc == 0 and "ERROR" not in err, err
        assert "# SUCCESS: correct in-place %dx%d->%d trilinear program (" % (case.na, case.nb, case.nc) in err and ") over %s " % field(q) in err, err
    else:
        assert rc == 1 and "SUCCESS" not in err, err
        assert "****** ERROR, not an in-place program of this triple over %s******" % field(q) in err
        e, where, got, exp = C.first_of(err)
        assert (e, where) == (want[1], case.where(want[1]))
        assert (got, exp) == (str(want[2]), str(want[3])), err
        if q:
            assert C.count_of(err) == (want[0], C.nequations(case))
        else:                                                                  # the count is that of the failing prime
            p = [p for _, _, p, t in C.passes_of(err) if t == "violated"]
            assert len(p) == 1 and C.count_of(err) == (C.definition(case, p[0])[0], C.nequations(case))
            assert "modulo %d: %d instead of %d" % ((p[0],) + C.definition(case, p[0])[2:]) in err
        rc2, err2 = C.tool(opts + paths, gpu, env=env)                         # without --count: the same first equation
        assert rc2 == 1 and C.first_of(err2) == (e, where, got, exp) and "equations violated" not in err2
    if q == 0:
        beta, j = C.certificate(case)
        gb, gj, primes = C.cert_of(err)
        assert gb >= beta and gb <= beta + 1 and gj == -(-gb // 30) and len(primes) == gj and primes[0] == C.P31
        assert gb >= C.cleared_defect_bits(case)
        ps = C.passes_of(err)
        assert [p for _, _, p, _ in ps] == primes[:len(ps)] and (len(ps) == gj or ps[-1][3] == "violated")
    return err


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_tool_against_definition(case, tmp_path):
    paths = case.write(tmp_path)
    for q in FIELDS:
        err = held_to_definition(case, paths, q)
        assert "# host: " in err or "ERROR: " in err
        assert "# GPU:" not in err
    if "hidden" in case.name:
        err = held_to_definition(case, paths, 0)
        assert [t for _, _, _, t in C.passes_of(err)] == ["no violated equation", "violated"]
        assert "found %d instead of 0; modulo" % C.P31 in err


def test_a_moduli_of_2_pow_31_and_more_is_announced(tmp_path):
    case = C.schoolbook(2, 5)
    rc, err = C.tool(["-q", C.P62] + case.write(tmp_path))
    assert rc == 0 and "# host:" in err
    rc, err = C.tool(["-q", 1 << 62] + case.write(tmp_path))                   # even: the lines /2 are no units
    assert rc == 4 and "is not invertible modulo" in err
    rc, err = C.tool(["-q", (1 << 62) + 1] + case.write(tmp_path))
    assert rc == 4 and "modulus above 2^62" in err


def test_more_than_64_primes_is_proved_over_q_on_the_host(tmp_path):
    """scalings by large numbers, undone: the certificate would take more than 64 primes"""
    base = C.schoolbook(2, 3)
    big = 10 ** 17 + 3
    text = "".join("a0:=a0*%d;\na0:=a0/%d;\n" % (big, big) for _ in range(40))
    for case, rc_want in ((base.with_text("big", text + base.text), 0), (base.with_text("bigbad", text + "a0:=a0*%d;\n" % big + base.text), 1)):
        assert C.certificate(case)[1] > 64
        rc, err = C.tool(["--count"] + case.write(tmp_path))
        assert rc == rc_want and "the proof is made over Q on the host" in err and "# host:" in err, err
        if rc_want:
            want = C.definition(case)
            assert C.first_of(err) == (want[1], case.where(want[1]), str(want[2]), str(want[3])) and C.count_of(err)[0] == want[0]


# ----------------------------------------------------------------------------- bin/trilplacer's own programs
def small_triples():
    """the SMALL rule of test_tril_oracle.py, restated"""
    out = []
    for l in sorted(glob.glob(os.path.join(DATA, "*_L.sms"))):
        r, p = l[:-6] + "_R.sms", l[:-6] + "_P.sms"
        if os.path.exists(r) and os.path.exists(p) and os.path.getsize(l) < 4000:
            try:
                for f in (l, r, p):
                    read_sms(f)
            except ValueError:
                continue
            out.append(os.path.basename(l)[:-6])
    return out


SMALL = small_triples()


def files(name):
    return [os.path.join(DATA, name + s) for s in ("_L.sms", "_R.sms", "_P.sms")]


def program(name, expanded=False):
    r = subprocess.run([TRILPLACER, "--gpu", "0", "-O", "3"] + (["-e"] if expanded else []) + files(name), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def printed_counts(name, expanded=False):
    """the (ADD, SCA, AXPY) that bin/trilplacer prints behind its program"""
    r = subprocess.run([TRILPLACER, "--gpu", "0", "-O", "3"] + (["-e"] if expanded else []) + files(name), capture_output=True, text=True, timeout=300)
    return [c for c, _ in re.findall(r"(?m)^# (\d+)\t(ADD|SCA|AXPY)", C.ANSI.sub("", r.stdout + r.stderr))[-3:]]


def is_matmul(name):
    """an AxBxC_* fixture whose tensor is the matrix-multiplication tensor (the -ALT and -CoB files hold an algorithm in another
    basis, or the change of basis itself)"""
    if not re.match(r"^\d+x\d+x\d+_", name):
        return False
    L, R, P = (read_sms(f) for f in files(name))
    try:
        return C.target(C.Case(name, L, R, P, "")) == C.target(C.Case(name, L, R, P, "", matmul=True))
    except (AssertionError, ZeroDivisionError):
        return False


def test_the_fixture_list():
    assert "4x4x4_48_rational" in SMALL and "2x2x2_7_Winograd" in SMALL and "1o1o2_3_Karatsuba" in SMALL and len(SMALL) >= 10


@pytest.mark.parametrize("name", SMALL)
def test_trilplacer_programs_are_certified(name, tmp_path):
    for expanded in (False, True):
        text = program(name, expanded)
        m, n, _ = read_sms(files(name)[0])
        nb, nc0 = read_sms(files(name)[1])[1], read_sms(files(name)[2])[0]
        recs = C.parse(text, n, nb, nc0 + int(expanded), expanded)             # the grammar is all that bin/trilplacer prints
        assert len(recs) == sum(1 for ln in text.splitlines() if ":=" in ln and not ln.startswith("#"))
        rc, err = C.tool((["-e"] if expanded else []) + files(name), stdin=text)
        assert rc == 0 and "# SUCCESS: correct in-place %dx%d->%d trilinear program (" % (n, nb, nc0 + int(expanded)) in err and ") over Q " in err, err
        counts = re.search(r"program \((\d+)\|(\d+)\|(\d+)\) over", err).groups()
        assert printed_counts(name, expanded) == list(counts)
        if is_matmul(name) and not expanded:
            rc, err = C.tool(["-m"] + files(name), stdin=text)
            assert rc == 0 and "SUCCESS" in err, err
            l, r, p = files(name)
            if n == nb:                                                        # a wrong triple of the same shape: B.A instead of A.B
                rc, err = C.tool([r, l, p], stdin=text)
                assert rc == 1 and "****** ERROR, not an in-place program of this triple over Q" in err and "SUCCESS" not in err, err
                assert C.first_of(err)[1].startswith("bilinear")


def test_a_wrong_triple_of_the_same_shape(tmp_path):
    """the Karatsuba program against a triple with one entry of P changed, and the Strassen program against -m of another shape"""
    text = program("1o1o2_3_Karatsuba")
    l, r, p = files("1o1o2_3_Karatsuba")
    m, n, ent = read_sms(p)
    (i, j), v = sorted(ent.items())[0]
    ent[(i, j)] = v + 1
    bad = C.Case("kbad", read_sms(l), read_sms(r), (m, n, ent), text)
    want = C.definition(bad)
    rc, err = C.tool(["--count"] + bad.write(tmp_path))
    assert rc == 1 and want[0] >= 1 and C.first_of(err)[0] == want[1] and C.count_of(err)[0] == want[0]
    for e in (False, True):
        rc, err = C.tool((["-e"] if e else []) + files("2o2o2_4_partSP"), stdin=program("2o2o2_5_shortproduct", e))
        assert rc == 1 and "SUCCESS" not in err and C.first_of(err)[1].startswith("bilinear (i,j,z) = (1,0,2)"), err   # the shapes agree, the maps differ


# ----------------------------------------------------------------------------- refusals and partial ranges
def test_refusals(tmp_path):
    case = C.schoolbook(2, 3)
    paths = case.write(tmp_path)
    for line, kind in C.REFUSED:
        rc, err = C.tool(paths[:3], stdin="# head\na0:=a0*3;\n" + line + "\n")
        assert rc == 4 and "line 3:" in err and (C.KINDS[kind] is None or C.KINDS[kind] in err) and "SUCCESS" not in err, (line, err)
    rc, err = C.tool(["-e"] + paths[:3], stdin="c0:=c0 + a0 * b0;\n")
    assert rc == 4 and "line 1:" in err and C.KINDS["plain"] in err
    rc, err = C.tool(["-q", 9] + paths)                                        # /3 modulo 9
    assert rc == 4 and "is not invertible modulo 9" in err and "line " in err
    frac = C.Case("frac", case.L, case.R, (case.P[0], case.P[1], {k: v / 5 for k, v in case.P[2].items()}), case.text)
    rc, err = C.tool(["-q", 35] + frac.write(tmp_path))
    assert rc == 4 and "a denominator (5) is not invertible modulo 35" in err
    rc, err = C.tool(["-m", "-e"] + paths)
    assert rc == 4 and "-m -e" in err
    rc, err = C.tool(["-m"] + paths)                                           # 2, 3, 4 is no m k, k n, m n
    assert rc == 4 and "are not m k, k n and m n" in err
    for rng in ("0:0", "6:1", "5:2"):
        rc, err = C.tool(["--pairs", rng] + paths)
        assert rc == 4 and "is empty or goes beyond the 6 pairs" in err
    rc, err = C.tool(["--pairs", "x"] + paths)
    assert rc == 4 and "--pairs needs first:count" in err
    other = C.schoolbook(2, 4).write(tmp_path)
    rc, err = C.tool([paths[0], other[1], paths[2], paths[3]])
    assert rc == 2 and "inner dimension mismatch" in err
    rc, err = C.tool(paths[:3] + [str(tmp_path / "none.prog")])
    assert rc == 4 and "cannot read" in err
    rc, err = C.tool([str(tmp_path / "none.sms")] + paths[1:])
    assert rc == 4 and "cannot read" in err


def tool_without_library(tmp_path):
    """a copy of the tool where no library is beside it, and an environment that names none"""
    import shutil
    os.makedirs(str(tmp_path / "alone" / "bin"), exist_ok=True)
    exe = shutil.copy(C.TPC, str(tmp_path / "alone" / "bin" / "TPchecker"))
    none = str(tmp_path / "alone" / "no_such_library.so")
    return exe, {"PLO_HIP_LIB": none, "PLINOPT_HIP_LIB": none, "LD_LIBRARY_PATH": ""}


def test_gpu_1_without_a_library_is_an_error(tmp_path):
    """--gpu 1 where the library cannot be loaded is an error, never the host loop"""
    exe, env = tool_without_library(tmp_path)
    case = C.schoolbook(2, 3)
    rc, err = C.tool(["-q", 131071] + case.write(tmp_path), gpu=1, env=env, exe=exe)
    assert rc == 4 and "libplinopt_hip.so cannot be loaded" in err and "# host:" not in err and "# GPU:" not in err and "SUCCESS" not in err, err
    assert C.tool(["-q", 131071] + case.write(tmp_path), gpu=0, env=env, exe=exe)[0] == 0


def test_the_choice_by_size(tmp_path):
    """without --gpu: the host loop below the crossover; above it the device, and where only the size chose the device and no
    library loads, the host loop, announced, with the verdict"""
    exe, env = tool_without_library(tmp_path)
    for case, rc_want in ((C.schoolbook(2, 5), 0), (C.mutations()[0][0], 1)):
        paths = case.write(tmp_path)
        rc, err = C.tool(["-q", 131071] + paths, gpu=None, env=dict(env, PLO_TPCHECKER_CROSSOVER="1e30"), exe=exe)
        assert rc == rc_want and "below the crossover of 1e+30: host loop" in err and "cannot be loaded" not in err and "# host: " in err, err
        rc, err = C.tool(["-q", 131071] + paths, gpu=None, env=dict(env, PLO_TPCHECKER_CROSSOVER="1"), exe=exe)
        assert rc == rc_want and "# --gpu not given: the size asks for the device, but libplinopt_hip.so cannot be loaded" in err, err
        assert ": host loop (--gpu 1 makes this an error)" in err and "# host: " in err and "# GPU:" not in err
        assert ("SUCCESS" in err) == (rc_want == 0)


def test_without_gpu_option_a_small_program_goes_to_the_host_loop(tmp_path):
    """the choice by size: far below the crossover the host loop runs, and says why"""
    case = C.schoolbook(2, 5)
    rc, err = C.tool(["-q", 131071] + case.write(tmp_path), gpu=None)
    assert rc == 0 and "# --gpu not given: " in err and "below the crossover" in err and "# host: " in err and "SUCCESS" in err


def test_partial_ranges(tmp_path):
    case = C.mutations()[4][0]                                                 # an AXPY sent to the wrong c: two violated equations
    paths = case.write(tmp_path)
    total = C.definition(case)
    pair = total[1] // case.w
    npairs = case.na * case.nb
    for q in (0, 131071):
        for p0, p1 in ((0, npairs), (pair, pair + 1), (0, pair), (pair + 1, npairs), (1, pair + 1)):
            want = C.definition(case, q, p0, p1)
            rc, err = C.tool((["-q", q] if q else []) + ["--count", "--pairs", "%d:%d" % (p0, p1 - p0)] + paths)
            note = "[partial: pairs %d .. %d of %d%s]" % (p0, p1 - 1, npairs, ", no restoration block" if p0 else "")
            assert note in err and rc == (1 if want[0] else 0), err
            if want[0]:
                assert C.first_of(err)[0] == want[1] and C.count_of(err) == (want[0], C.nequations(case, p0, p1))
    ra = C.mutations()[5][0]                                                   # a restoration block goes with the ranges from pair 0
    paths = ra.write(tmp_path)
    assert C.tool(["--pairs", "0:1"] + paths)[0] == 1 and C.tool(["--pairs", "1:2"] + paths)[0] == 0
