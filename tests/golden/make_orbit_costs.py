"""Writes tests/golden/orbit_costs.json: the per-seed (cost, nnz, nno) of the De Groote orbit search (bin/orbiter,
reference src/orbiter.cpp:272-324), computed by the literal oracle tests/orbit_oracle.py.

  fixtures   "name|modulus|measure" -> [out3 of PLO_ORBIT_BASE_SEED, then of SEEDS], for
             every shape-valid rational triple of tests/golden/data over Q with -s (measure 0) and with -c (measure 2);
             SUBSET over Z_131071 and Z_3 (density; a triple with a denominator divisible by the modulus is left out); 2x2x2_7_DPS-accurate modulo (1013^2 - 3)/2 = 513083 (`-r 1013 2 3`)
  long       4x4x4_49_156 over Q with -s: seeds 0 .. LONG-1, flattened 3 per seed

Run from the repository root: python tests/golden/make_orbit_costs.py  (under a minute on 8 cores)."""
import glob
import json
import os
import sys
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import orbit_oracle as O  # noqa: E402
from plo_testlib import DATA  # noqa: E402

SEEDS = list(range(32))
SUBSET = ["2x2x2_7_Strassen", "2x2x2_7_Winograd", "3x3x3_23_58", "3x4x7_63_rational", "4x4x4_48_rational", "4x4x4_49_156", "6x3x3_40"]
LONG_NAME, LONG = "4x4x4_49_156", 10000
MOD_DPS = (1013 ** 2 - 3) // 2           # `-r 1013 2 3`: the factor 2 removed, as the tool does


def triples():
    """the shape-valid rational triples of tests/golden/data"""
    out = []
    for f in sorted(glob.glob(os.path.join(DATA, "*_L.sms"))):
        b = f[:-6]
        if not all(os.path.exists(b + "_%s.sms" % x) for x in "RP"):
            continue
        try:
            _, sh = O.load(b)
        except ValueError:                     # symbolic placeholders (-X_): not rational
            continue
        if sh is not None:
            out.append(os.path.basename(b))
    return out


def invertible(name, p):
    """every denominator of the triple is a unit modulo p (the tool refuses the others)"""
    mats, _ = O.load(os.path.join(DATA, name))
    return all(getattr(x, "denominator", 1) % p for M in mats if not hasattr(M, "dtype") for row in M for x in row)


def job(arg):
    name, mod, measure, seeds = arg
    mats, sh = O.load(os.path.join(DATA, name))
    return [list(O.cost3(mats, sh, s, modulus=mod, measure=measure)) for s in seeds]


def main():
    names = triples()
    seeds = [O.BASE_SEED] + SEEDS
    jobs = [(nm, 0, ms, seeds) for nm in names for ms in (O.DENSITY, O.CANONICAL)]
    jobs += [(nm, p, O.DENSITY, seeds) for nm in SUBSET for p in (131071, 3) if invertible(nm, p)]
    jobs += [("2x2x2_7_DPS-accurate", MOD_DPS, O.DENSITY, seeds)]
    chunks = [(LONG_NAME, 0, O.DENSITY, list(range(s, min(s + 500, LONG)))) for s in range(0, LONG, 500)]
    with Pool() as p:
        res = p.map(job, jobs + chunks, chunksize=1)
    fx = {"%s|%d|%d" % (nm, mod, ms): r for (nm, mod, ms, _), r in zip(jobs, res)}
    long_out = [x for r in res[len(jobs):] for c in r for x in c]
    out = {
        "stream": "include/plinopt_hip.h PLO_ORBIT_*: CandRng; U, then V, then W: Fisher-Yates P, Q, the signs, the strict upper part",
        "base_seed": O.BASE_SEED, "seeds": SEEDS, "triples": names,
        "fixtures": fx,
        "long": {"name": LONG_NAME, "modulus": 0, "measure": 0, "seed0": 0, "n": LONG, "out3": long_out},
    }
    with open(os.path.join(HERE, "orbit_costs.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(len(fx), "fixture entries;", len(names), "triples")


if __name__ == "__main__":
    main()
