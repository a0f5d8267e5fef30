"""The De Groote orbit search on the MI355X (plo_orbit.hip through plo_orbit_*): per-seed counts bit-exact against
tests/golden/orbit_costs.json (the literal oracle tests/orbit_oracle.py), the search's argmin against the golden minimum,
bin/orbiter --gpu 1 against --gpu 0 (winner line and written files byte for byte), the announced host loop for inputs the
device refuses, the sharded search, and a long search whose winner replays on the host."""
import json
import os
import shutil
import subprocess

import pytest

from plo_testlib import DATA, GOLDEN, ROOT, read_sms

pytestmark = pytest.mark.gpu

ORB = os.path.join(ROOT, "bin", "orbiter")
GOLD = json.load(open(os.path.join(GOLDEN, "orbit_costs.json")))
BASE = (1 << 64) - 1


def run(cmd, timeout=300):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout, r.stderr


def files(name, d=DATA):
    return [os.path.join(d, "%s_%s.sms" % (name, x)) for x in "LRP"]


def csr_of(path):
    m, n, e = read_sms(path)
    rp, col, num, den = [0], [], [], []
    for i in range(m):
        for j in sorted(jj for (ii, jj) in e if ii == i):
            col.append(j); num.append(e[(i, j)].numerator); den.append(e[(i, j)].denominator)
        rp.append(len(col))
    return m, n, rp, col, num, den


def triple(name, d=DATA):
    return [csr_of(f) for f in files(name, d)]


def plan(name, modulus=0, measure=0):
    from plinopt_amd import OrbitPlan
    return OrbitPlan(*triple(name), modulus=modulus, measure=measure)


def test_cost_many_bit_exact_every_entry(hip):
    seeds = [BASE] + GOLD["seeds"]
    for key in sorted(GOLD["fixtures"]):
        name, mod, ms = key.split("|")
        got = [list(c) for c in plan(name, int(mod), int(ms)).cost_many(seeds)]
        assert got == GOLD["fixtures"][key], key


def test_cost_many_long_run_bit_exact(hip):
    L = GOLD["long"]
    got = [x for c in plan(L["name"]).cost_many(seed0=L["seed0"], n=L["n"]) for x in c]
    assert got == L["out3"]


def test_search_argmin_ten_thousand_seeds(hip):
    L = GOLD["long"]
    o = L["out3"]
    want = min((o[3 * j], o[3 * j + 1], o[3 * j + 2], L["seed0"] + j) for j in range(L["n"]))
    (c, z, q), seed = plan(L["name"]).search(L["seed0"], L["n"])
    assert (c, z, q, seed) == want


def nnz_files(src):
    return [p[:-4] + ".nnz.sms" for p in src]


def gpu_vs_host(name, args, tmp_path):
    out = {}
    for g in ("1", "0"):
        d = tmp_path / ("g" + g)
        d.mkdir()
        for f in files(name):
            shutil.copy(f, d)
        src = files(name, str(d))
        rc, so, se = run([ORB, "--gpu", g] + args + src)
        assert rc == 0, se
        out[g] = (so, se, [open(p, "rb").read() if os.path.exists(p) else None for p in nnz_files(src)])
    assert out["1"][0] == out["0"][0]
    assert out["1"][2] == out["0"][2]
    assert "restarts on host" in out["0"][1]
    return out


@pytest.mark.parametrize("name,args", [("2x2x2_7_Winograd", ["-O", "300"]), ("4x4x4_48_rational-CoB", ["-c", "-O", "200"]),
                                       ("3x3x3_23_58", ["-m", "3", "-O", "100"]), ("4x4x4_49_156", ["--seed", "5", "-O", "2000"]),
                                       ("2x2x2_7_DPS-accurate", ["-r", "1013", "2", "3", "-O", "500"]),
                                       ("3x4x7_63_rational", ["-O", "300"])])
def test_cli_gpu_equals_host(hip, name, args, tmp_path):
    out = gpu_vs_host(name, args, tmp_path)
    assert "restarts on GPU" in out["1"][1]


def test_wide_modulus_is_refused_and_runs_on_host(hip, tmp_path):
    from plinopt_amd import OrbitPlan, capi
    with pytest.raises(capi.PloError) as ex:
        OrbitPlan(*triple("2x2x2_7_Strassen"), modulus=2147483659)
    assert ex.value.code == capi.PLO_E_UNSUPPORTED
    out = gpu_vs_host("2x2x2_7_Strassen", ["-m", "2147483659", "-O", "200"], tmp_path)
    assert "host search" in out["1"][1] and "restarts on host" in out["1"][1]


def test_int64_bound_is_refused_and_runs_on_host(hip, tmp_path):
    """a row of L whose L1 norm passes 2^62: plo_orbit_plan_create_q refuses it (PLO_E_UNSUPPORTED), the tool says so"""
    from plinopt_amd import OrbitPlan, capi
    src = tmp_path / "src"
    src.mkdir()
    for f in files("2x2x2_7_Strassen"):
        shutil.copy(f, src)
    lf = src / "2x2x2_7_Strassen_L.sms"
    lines = [ln for ln in lf.read_text().splitlines() if ln.strip() and not ln.startswith("#")]
    lines.insert(1, "1 2 4611686018427387903")
    lines.insert(2, "1 3 4611686018427387903")
    lf.write_text("\n".join(lines) + "\n")
    with pytest.raises(capi.PloError) as ex:
        OrbitPlan(*triple("2x2x2_7_Strassen", str(src)))
    assert ex.value.code == capi.PLO_E_UNSUPPORTED
    outs = {}
    for g in ("1", "0"):
        d = tmp_path / ("g" + g)
        shutil.copytree(src, d)
        rc, so, se = run([ORB, "--gpu", g, "-O", "100"] + files("2x2x2_7_Strassen", str(d)))
        assert rc == 0, se
        outs[g] = (so, se, [open(p, "rb").read() if os.path.exists(p) else None for p in nnz_files(files("2x2x2_7_Strassen", str(d)))])
    assert "host search" in outs["1"][1]
    assert outs["1"][0] == outs["0"][0] and outs["1"][2] == outs["0"][2]


def test_search_multi_shards_equal_one_device(hip):
    from plinopt_amd import orbit_search_multi
    args = triple("4x4x4_49_156")
    one = plan("4x4x4_49_156").search(1000, 3001)
    for nd in (1, 2, 3):
        got, st = orbit_search_multi(*args, 0, 0, 1000, 3001, [0] * nd)
        assert got == one, nd
        assert st["candidates"] == 3001


def test_million_candidates_winner_replays_on_host(hip):
    name = "3x4x7_63_rational"
    P = plan(name)
    (c, z, q), seed = P.search(0, 1000000)
    assert P.last_stats["candidates"] == 1000000
    rc, out, err = run([ORB, "--gpu", "0", "--costs", "--seed", str(seed), "-O", "1"] + files(name))
    assert rc == 0, err
    assert [int(x) for x in out.splitlines()[1].split()] == [c, z, q]
