"""The in-place linear search on the MI355X (plo_lin.hip through plo_lin_*): per-seed counts bit-exact against
tests/golden/lin_costs.json (the literal oracle tests/lin_oracle.py), the search's argmin against the host order, bin/inplacer
--gpu 1 against --gpu 0 byte for byte, the announced host loop for a row the kernel refuses, and the sharded search."""
import json
import os
import subprocess

import pytest

from plo_testlib import DATA, GOLDEN, ROOT, read_sms

pytestmark = pytest.mark.gpu

INP = os.path.join(ROOT, "bin", "inplacer")
CHK = os.path.join(ROOT, "bin", "SLPchecker")
GOLD = json.load(open(os.path.join(GOLDEN, "lin_costs.json")))
BASE = (1 << 64) - 1


def run(cmd, stdin=None, timeout=240):
    r = subprocess.run(cmd, input=stdin, capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout, r.stderr


def csr(name, transposed=False):
    m, n, e = read_sms(os.path.join(DATA, name + ".sms"))
    if transposed:
        m, n, e = n, m, {(j, i): v for (i, j), v in e.items()}
    rp, col, num, den = [0], [], [], []
    for i in range(m):
        for j in sorted(jj for (ii, jj) in e if ii == i):
            col.append(j); num.append(e[(i, j)].numerator); den.append(e[(i, j)].denominator)
        rp.append(len(col))
    return m, n, rp, col, num, den


def plan(name, transposed=False):
    from plinopt_amd import LinPlan
    return LinPlan(*csr(name, transposed))


def test_cost_many_bit_exact_every_fixture(hip):
    seeds = [BASE] + GOLD["seeds"]
    for key in sorted(GOLD["fixtures"]):
        name, how = key.split("|")
        got = [list(a) + list(b) for a, b in plan(name, how == "t").cost_many(seeds)]
        assert got == GOLD["fixtures"][key], key


def test_cost_many_long_run_bit_exact(hip):
    L = GOLD["long"]
    P = plan(L["name"])
    got = [x for a, b in P.cost_many(seed0=L["seed0"], n=L["n"]) for x in list(a) + list(b)]
    assert got == L["ops"]


def test_search_same_argmin_ten_thousand_seeds(hip):
    L = GOLD["long"]
    ops = L["ops"]
    want = min((ops[6 * k + 3 * v], ops[6 * k + 3 * v + 1], L["seed0"] + k, v) for k in range(L["n"]) for v in (0, 1))
    (a, s, r), seed, var = plan(L["name"]).search(L["seed0"], L["n"])
    assert (a, s, seed, var) == want
    assert r == ops[6 * (seed - L["seed0"]) + 3 * var + 2]


@pytest.mark.parametrize("name,tr,seed,loops", [("4x4x4_49_156_L", False, 5, 300), ("2o2o2_4_partSP_L", True, 0, 200),
                                                ("3x4x7_63_rational_L", False, 9, 100), ("4x4x4_48_rational_P", True, 3, 100)])
def test_cli_gpu_equals_host(hip, name, tr, seed, loops, tmp_path):
    f = os.path.join(DATA, name + ".sms")
    args = ["--seed", str(seed), "-O", str(loops), f] + (["-t"] if tr else [])
    rc1, g, e1 = run([INP, "--gpu", "1"] + args)
    assert rc1 == 0, e1
    assert "restarts on GPU" in e1
    rc0, h, e0 = run([INP, "--gpu", "0"] + args)
    assert rc0 == 0, e0
    assert g == h
    if tr:
        m, n, e = read_sms(f)
        t = tmp_path / "T.sms"
        t.write_text("%d %d R\n" % (n, m) + "".join("%d %d %s\n" % (j + 1, i + 1, v) for (i, j), v in sorted(e.items())) + "0 0 0\n")
        f = str(t)
    rc, _, e2 = run([CHK, "-M", f], stdin=g)
    assert rc == 0 and "SUCCESS" in e2, e2


def test_long_row_runs_the_announced_host_loop(hip, tmp_path):
    """a row of more than 64 entries: plo_lin_plan_create_q refuses it (PLO_E_UNSUPPORTED), the tool says so and runs the
    host loop; the text is the host's"""
    from plinopt_amd import LinPlan, capi
    m, n = 3, 70
    ent = [(0, j, 1 if j % 3 else -1) for j in range(70)] + [(1, 0, 1), (1, 5, 2)] + [(2, j, 1) for j in range(0, 70, 7)]
    f = tmp_path / "long.sms"
    f.write_text("%d %d R\n" % (m, n) + "".join("%d %d %d\n" % (i + 1, j + 1, v) for i, j, v in ent) + "0 0 0\n")
    rp, col, num = [0], [], []
    for i in range(m):
        for (ii, j, v) in ent:
            if ii == i:
                col.append(j); num.append(v)
        rp.append(len(col))
    with pytest.raises(capi.PloError) as ex:
        LinPlan(m, n, rp, col, num)
    assert ex.value.code == capi.PLO_E_UNSUPPORTED
    rc1, g, e1 = run([INP, "--gpu", "1", "--seed", "2", "-O", "50", str(f)])
    assert rc1 == 0, e1
    assert "host search" in e1 and "restarts on host" in e1
    rc0, h, e0 = run([INP, "--gpu", "0", "--seed", "2", "-O", "50", str(f)])
    assert rc0 == 0 and g == h
    rc, _, e2 = run([CHK, "-M", str(f)], stdin=g)
    assert rc == 0 and "SUCCESS" in e2


def test_search_multi_shards_equal_one_device(hip):
    """plo_lin_search_multi with 1, 2 and 3 shards (duplicate ordinals on a one-GPU box) == one device"""
    from plinopt_amd import lin_search_multi
    args = csr("4x4x4_49_156_L")
    one = plan("4x4x4_49_156_L").search(1000, 3001)
    for nd in (1, 2, 3):
        got, st = lin_search_multi(*args, 1000, 3001, [0] * nd)
        assert got == one, nd
        assert st["candidates"] == 3001
