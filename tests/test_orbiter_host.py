"""bin/orbiter on the host (--gpu 0), held to the literal oracle tests/orbit_oracle.py and to tests/golden/orbit_costs.json:
per-seed counts of every shape-valid fixture triple, the files a search writes (only when it improves, exact Brent equations,
counts that match the winner line, byte-identical reruns), the modulus conventions of the reference and the refusals."""
import json
import os
import shutil
import subprocess

import pytest

import orbit_oracle as O
from plo_testlib import DATA, GOLDEN, ROOT, read_sms

ORB = os.path.join(ROOT, "bin", "orbiter")
GOLD = json.load(open(os.path.join(GOLDEN, "orbit_costs.json")))


def run(cmd, timeout=300):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    return r.returncode, r.stdout, r.stderr


def files(name, d=DATA):
    return [os.path.join(d, "%s_%s.sms" % (name, x)) for x in "LRP"]


def field_args(mod, ms):
    return (["-m", mod] if mod != "0" else []) + (["-c"] if ms == "2" else [])


def copies(name, tmp_path):
    for f in files(name):
        shutil.copy(f, tmp_path)
    return files(name, str(tmp_path))


def winner(out):
    line = [ln for ln in out.splitlines() if ln.startswith("winner ")]
    assert len(line) == 1, out
    t = line[0].split()
    return int(t[1]), int(t[2]), int(t[3]), t[4]


def test_golden_covers_every_shape_valid_triple():
    assert len(GOLD["triples"]) == 28
    for nm in GOLD["triples"]:
        for ms in (0, 2):
            assert "%s|0|%d" % (nm, ms) in GOLD["fixtures"]
    assert "2x2x2_7_DPS-accurate|513083|0" in GOLD["fixtures"]
    assert any(k.endswith("|3|0") for k in GOLD["fixtures"]) and any(k.endswith("|131071|0") for k in GOLD["fixtures"])


def test_costs_equal_golden_every_entry():
    n = len(GOLD["seeds"])
    assert GOLD["seeds"] == list(range(n))
    for key, want in sorted(GOLD["fixtures"].items()):
        name, mod, ms = key.split("|")
        rc, out, err = run([ORB, "--gpu", "0", "--costs", "-O", str(n)] + field_args(mod, ms) + files(name))
        assert rc == 0, err
        assert [list(map(int, ln.split())) for ln in out.splitlines()] == want, key


def test_costs_equal_golden_long_run():
    L = GOLD["long"]
    rc, out, err = run([ORB, "--gpu", "0", "--costs", "--seed", str(L["seed0"]), "-O", str(L["n"])] + files(L["name"]))
    assert rc == 0, err
    lines = out.splitlines()
    assert len(lines) == L["n"] + 1
    assert [int(x) for ln in lines[1:] for x in ln.split()] == L["out3"]


def test_oracle_equals_golden_few_seeds():
    """the Fraction oracle recomputes the base candidate and one seed of every golden entry"""
    cache = {}
    for key, want in sorted(GOLD["fixtures"].items()):
        name, mod, ms = key.split("|")
        if name not in cache:
            cache[name] = O.load(os.path.join(DATA, name))
        mats, sh = cache[name]
        j = 1 + (sum(map(ord, key)) % len(GOLD["seeds"]))
        for idx, seed in ((0, O.BASE_SEED), (j, GOLD["seeds"][j - 1])):
            assert list(O.cost3(mats, sh, seed, modulus=int(mod), measure=int(ms))) == want[idx], (key, seed)


def sms_mats(paths):
    mats = [read_sms(p) for p in paths]
    return [O.dense(*t) for t in mats]


@pytest.mark.parametrize("name,args,improves", [
    ("2x2x2_7_Winograd", ["-O", "300"], True),
    ("2x2x2_7_Winograd", ["-c", "-O", "300"], False),
    ("4x4x4_48_rational-CoB", ["-c", "-O", "100"], True),
    ("3x3x3_23_58", ["-m", "3", "-O", "100"], False),
    ("4x4x4_48_rational-CoB", ["-m", "3", "-O", "60", "--seed", "7"], True),
    ("2x2x2_7_DPS-accurate", ["-r", "1013", "2", "3", "-O", "200"], None),
])
def test_search_writes_only_improvements(name, args, improves, tmp_path):
    src = copies(name, tmp_path)
    rc, out, err = run([ORB, "--gpu", "0"] + args + src)
    assert rc == 0, err
    assert "restarts on host" in err and "Search(" in err and "Init. ops" in err
    cost, nnz, nno, seed = winner(out)
    outs = [p[:-4] + ".nnz.sms" for p in src]
    mod = 0
    if "-m" in args:
        mod = int(args[args.index("-m") + 1])
    if "-r" in args:
        mod = 513083
    ms = O.CANONICAL if "-c" in args else O.DENSITY
    mats_in, sh = O.load(os.path.join(str(tmp_path), name))
    base = O.cost3(mats_in, sh, O.BASE_SEED, modulus=mod, measure=ms)
    if seed == "base":
        assert improves in (False, None)
        assert (cost, nnz, nno) == base
        assert not any(os.path.exists(p) for p in outs)
        return
    assert improves in (True, None)
    assert (cost, nnz, nno) < base and "Rdcd. opt" in err
    assert all(os.path.exists(p) for p in outs)
    got = sms_mats(outs)
    assert O.counts(*got, modulus=mod, measure=ms) == (cost, nnz, nno)
    if O.mm_check(*mats_in, sh, modulus=mod):
        assert O.mm_check(*got, sh, modulus=mod)
    first = [open(p, "rb").read() for p in outs]
    for p in outs:
        os.remove(p)
    rc2, out2, err2 = run([ORB, "--gpu", "0"] + args + src)
    assert rc2 == 0 and out2 == out
    assert [open(p, "rb").read() for p in outs] == first


def test_winner_replays_as_candidate(tmp_path):
    """--candidate writes the matrices of one candidate; the oracle's products of the same seed are equal"""
    name = "2x2x2_7_Strassen"
    rc, _, err = run([ORB, "--gpu", "0", "--candidate", "11", str(tmp_path / "c")] + files(name))
    assert rc == 0, err
    got = sms_mats([str(tmp_path / "c" / (x + ".sms")) for x in "LRP"])
    mats, sh = O.load(os.path.join(DATA, name))
    want = [[[x for x in row] for row in (M.tolist() if hasattr(M, "tolist") else M)] for M in O.products(mats, sh, 11)]
    assert [[list(r) for r in M] for M in got] == want
    assert O.mm_check(*got, sh)


@pytest.mark.parametrize("args,field", [(["-m", "12"], "Z/3Z"), (["-m", "8"], "Z/2Z"), (["-q", "131071"], "Z/131071Z"),
                                        (["-r", "1013", "2", "3"], "Z/513083Z"), ([], "over Q")])
def test_modulus_parsing(args, field):
    rc, out, err = run([ORB, "--gpu", "0", "-O", "3"] + args + files("2x2x2_7_Strassen"))
    assert rc == 0, err
    assert field in err


def test_dps_accurate_is_mm_only_modulo_513083():
    rc, _, err = run([ORB, "--gpu", "0", "-O", "0"] + files("2x2x2_7_DPS-accurate"))
    assert rc == 0 and "ERROR, not a 2x2x2 MM algorithm" in err
    rc, _, err = run([ORB, "--gpu", "0", "-O", "0", "-r", "1013", "2", "3"] + files("2x2x2_7_DPS-accurate"))
    assert rc == 0 and "SUCCESS: correct 2x2x2" in err


@pytest.mark.parametrize("args", [["-z"], ["-P", "X^2-3"], ["-I", "Y"], ["-m", "3"], ["-m", "18446744073709551615"], ["-r", "2", "64", "1"], ["shapes"]])
def test_refusals_exit_2(args, tmp_path):
    f = files("2x2x2_7_DPS-accurate")
    if args == ["shapes"]:
        args, f = [], [f[0]] + files("3x3x3_23_58")[1:]
    rc, out, err = run([ORB, "--gpu", "0", "-O", "5"] + args + f)
    assert rc == 2, (rc, err)
    assert "ERROR" in err and not out
    assert not any(os.path.exists(p[:-4] + ".nnz.sms") for p in f)
