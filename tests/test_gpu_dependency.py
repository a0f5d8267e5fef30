"""The row-dependency enumeration on the GPU (plo_dep.hip, plo_dep_*, bin/dependency --gpu 1), held to the literal oracle
tests/dependency_oracle.py through tests/golden/dependency_hits.json: the hit list of DepPlan (over Q after the caller's
filter), the tool's text against its own host loop, the synthetic shapes at which the kernel takes another path, the
superset filter over Q, the announced refusals, and a matrix too large for LDS at the limits the C-ABI promises."""
import hashlib
import json
import os
import subprocess

import pytest

import dependency_oracle as D
from plo_testlib import DATA, GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEP = os.path.join(ROOT, "bin", "dependency")
GOLD = json.load(open(os.path.join(GOLDEN, "dependency_hits.json")))
CASES = [r for r in GOLD["fixtures"] + GOLD["synthetic"] if r["l"] != 0]      # -l 0 stays on the host
SYN = {(r["input"], r["q"]): r for r in GOLD["synthetic"]}
P31 = 2147483629


def run(cmd, timeout=120):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout, r.stderr


def case_id(rec):
    return "%s-l%d-c%d-q%d%s" % (rec["input"], rec["l"], rec["c"], rec["q"], "-v" if rec["v"] else "")


def args_of(rec):
    return ["-l", str(rec["l"]), "-c", str(rec["c"])] + (["-q", str(rec["q"])] if rec["q"] else []) + (["-v", rec["v"]] if rec["v"] else [])


def matrix_of(rec):
    if "sms" in rec:
        return D.parse_sms(rec["sms"])
    return D.load_sms(os.path.join(DATA, rec["input"] + ".sms"))


def input_of(rec, tmp_path):
    if "sms" not in rec:
        return os.path.join(DATA, rec["input"] + ".sms")
    p = tmp_path / (rec["input"] + ".sms")
    p.write_text(rec["sms"])
    return str(p)


def same_text(out, rec):
    if "text" in rec:
        assert out == rec["text"]
    assert out.count("\n") == rec["lines"]
    assert hashlib.sha256(out.encode()).hexdigest() == rec["sha256"]


def csr_of(rows):
    rp, col, num, den = [0], [], [], []
    for r in rows:
        for j, x in r:
            col.append(j); num.append(x.numerator); den.append(x.denominator)
        rp.append(len(col))
    return rp, col, num, den


def plan_of(rec, hip):
    """(plan, field, field matrix, FCoeffs) of a golden case: the coefficient list is the caller's, as in the tool"""
    from plinopt_amd import DepPlan
    m, n, rows = matrix_of(rec)
    F = D.field(rec["q"])
    C = D.rational_coefficients(rows, rec["v"].split(), rec["c"])
    FC, pairs = [], []
    for e in C:
        x = F.image(e)
        if x is not None and x != F.zero and x not in FC:
            FC.append(x)
            pairs.append((x, 1) if rec["q"] else (e.numerator, e.denominator))
    rp, col, num, den = csr_of(rows)
    return DepPlan(m, n, rp, col, num, den, coeffs=pairs, modulus=rec["q"], level=rec["l"]), F, D.field_matrix(F, rows), FC, n


@pytest.mark.parametrize("rec", CASES, ids=case_id)
def test_plan_hits_equal_golden(hip, rec):
    """every hit recomputed in the field: over Z_q the device's verdict must be the field's, over Q a reported combination
    may be false (it is dropped) but the surviving text is the golden one, in order"""
    plan, F, M, FC, n = plan_of(rec, hip)
    hits = plan.search()
    assert plan.last_nhits == len(hits)
    lines = []
    for rows, idx, kind, col, residue in hits:
        W = D.combination(F, M, n, FC, rows, idx)
        ln = D.line_of(F, FC, rows, idx, W)
        if rec["q"]:
            nz = [j for j, x in enumerate(W) if x != 0]
            assert ln is not None and kind == len(nz)
            if kind == 1:
                assert (col, residue) == (nz[0], W[nz[0]])
        if ln is not None:
            lines.append(ln + "\n")
    same_text("".join(lines), rec)
    if not rec["q"] and not rec["input"].startswith("filter"):
        assert len(lines) == len(hits)                    # nothing in these inputs vanishes modulo the prime only


@pytest.mark.parametrize("rec", CASES, ids=case_id)
def test_tool_gpu_equals_host(rec, tmp_path):
    f = input_of(rec, tmp_path)
    rc, out, err = run([DEP, "--gpu", "1"] + args_of(rec) + [f])
    assert rc == 0, err
    assert "combinations on GPU" in err and "host search" not in err
    rc0, out0, err0 = run([DEP, "--gpu", "0"] + args_of(rec) + [f])
    assert rc0 == 0 and out == out0
    same_text(out, rec)
    assert rec["head"] in err.splitlines()


def test_capacity_reports_the_full_count(hip):
    from plinopt_amd import capi
    rec = SYN[("n1_m12", 0)]
    plan, F, M, FC, n = plan_of(rec, hip)
    full = plan.search(cap=4096)
    assert len(full) == 2178 == rec["lines"]               # n = 1: every combination is a hit
    with pytest.raises(capi.PloError) as e:
        plan.search(cap=100)
    assert e.value.code == capi.PLO_E_CAPACITY and plan.last_nhits == 2178
    assert plan.search(cap=2178) == full
    assert plan.search(row0=3, row1=5, cap=2178) == [h for h in full if h[0][0] in (3, 4)]


def test_superset_filter(hip, tmp_path):
    from plinopt_amd import DEP_ZERO
    # (1, p+1, 2p+1) - (1, 1, 1) vanishes modulo p only: the device reports it, the tool prints nothing
    rec = SYN[("filter_false_hit", 0)]
    plan, F, M, FC, n = plan_of(rec, hip)
    assert plan.search() == [((0, 1), (None, 1), DEP_ZERO, 0, 0)] and FC[1] == -1
    rc, out, err = run([DEP, "--gpu", "1"] + args_of(rec) + [input_of(rec, tmp_path)])
    assert rc == 0 and out == "" and "on GPU" in err
    # (1, p+1) - (1, 1) = (0, p): zero for the device, canonical over Q
    rec = SYN[("filter_zero_is_canonical", 0)]
    plan, F, M, FC, n = plan_of(rec, hip)
    assert plan.search() == [((0, 1), (None, 1), DEP_ZERO, 0, 0)]
    rc, out, err = run([DEP, "--gpu", "1"] + args_of(rec) + [input_of(rec, tmp_path)])
    assert rc == 0 and out == "-i1*%d+o0-o1;\n" % P31 and "on GPU" in err


@pytest.mark.parametrize("extra", [["-q", "2147483659", "-l", "3"], ["-l", "9", "-c", "3"]], ids=["modulus-2^31", "level-9"])
def test_refusals_run_on_the_host(extra):
    f = os.path.join(DATA, "2x2x2_7_Winograd_L.sms")
    rc, out, err = run([DEP, "--gpu", "1"] + extra + [f])
    assert rc == 0, err
    assert "the device refuses this input" in err and "host search" in err and "combinations on host" in err
    rc0, out0, err0 = run([DEP, "--gpu", "0"] + extra + [f])
    assert rc0 == 0 and out == out0 and out


def test_refusal_codes(hip):
    from plinopt_amd import DepPlan, capi
    for kw in (dict(level=9), dict(modulus=1 << 31), dict(coeffs=((1, P31),))):
        with pytest.raises(capi.PloError) as e:
            DepPlan(2, 2, [0, 1, 2], [0, 1], [1, 1], **kw)
        assert e.value.code == capi.PLO_E_UNSUPPORTED, kw
    with pytest.raises(capi.PloError) as e:
        DepPlan(2, 2, [0, 1, 2], [0, 1], [1, 1], [1, P31])  # a denominator of the matrix that vanishes modulo the prime
    assert e.value.code == capi.PLO_E_UNSUPPORTED


def test_larger_run_gpu_equals_host():
    f = os.path.join(DATA, "4x4x4_49_156_L.sms")
    a = ["-l", "4", "-c", "3", f]
    rc, out, err = run([DEP, "--gpu", "1"] + a)
    assert rc == 0 and "combinations on GPU" in err, err
    rc0, out0, err0 = run([DEP, "--gpu", "0"] + a)
    assert rc0 == 0 and out == out0 and out.count("\n") > 250


def big_matrix(p, planted):
    """512 x 128 residues (too large for LDS: the kernel reads it through L2); `planted` writes the last row"""
    s, rows = 12345, []
    for _ in range(512):
        r = []
        for _ in range(128):
            s = (s * 1103515245 + 12345) % (1 << 31)
            r.append(1 + (s >> 8) % (p - 1))
        rows.append(r)
    rows[511] = planted(rows)
    return rows


@pytest.mark.parametrize("ncoef,row0", [(64, 509), (3, 505)], ids=["64-coefficients", "six-deep"])
def test_promised_limits_and_matrix_outside_lds(hip, ncoef, row0):
    """512 x 128, level 6, 64 coefficients is admitted; its last top rows equal the oracle on the same rows.  With 3
    coefficients the walk under row 505 is six rows deep and ends on a planted combination of six rows."""
    from plinopt_amd import DepPlan
    p = 131071
    fc = list(range(1, ncoef + 1))
    if ncoef == 64:                                       # o509 + 6 o510 + 10 o511 = 0 but for column 77
        def planted(R):
            v = [(-(a + fc[5] * b) * pow(fc[9], -1, p)) % p for a, b in zip(R[509], R[510])]
            v[77] = (v[77] + 1) % p
            return v
    else:                                                 # o505 + o507 + 2 o508 + 3 o509 + o510 + 2 o511 = 0
        def planted(R):
            return [(-(a + fc[0] * b + fc[1] * c + fc[2] * d + fc[0] * e) * pow(fc[1], -1, p)) % p for a, b, c, d, e in zip(R[505], R[507], R[508], R[509], R[510])]
    rows = big_matrix(p, planted)
    rp = [128 * i for i in range(513)]
    plan = DepPlan(512, 128, rp, list(range(128)) * 512, [x for r in rows for x in r], coeffs=[(c, 1) for c in fc], modulus=p, level=6)
    got = plan.search(row0=row0, row1=512)
    sub = [[(j, D.Fraction(x)) for j, x in enumerate(r)] for r in rows[row0:]]
    _, want = D.depender(512 - row0, 128, sub, level=6, q=p, fc=fc)
    want = [(tuple(r + row0 for r in h[0]), h[1], h[2], h[3] if h[2] else 0, (-h[4]) % p) for h in want]
    assert got == want and len(got) >= 1
    if ncoef == 3:
        assert ((505, 507, 508, 509, 510, 511), (None, 0, 1, 2, 0, 1), 0, 0, 0) in got
    else:
        assert ((509, 510, 511), (None, 5, 9), 1, 77, fc[9]) in got
