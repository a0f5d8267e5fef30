"""Writes tests/golden/lin_costs.json: the per-seed (ADD, SCA, ROWS) of variant 0 and of variant 1 of the in-place linear
search (bin/inplacer, reference include/plinopt_inplace.inl:604-673), computed by the literal oracle tests/lin_oracle.py.

  fixtures   every rational data matrix, direct ("name|d") and transposed as `inplacer -t` searches it ("name|t"):
             the candidates BASE_SEED (the unpermuted oriented program, both halves equal) and SEEDS
  long       4x4x4_49_156_L, direct: seeds 0 .. LONG-1, flattened 6 per seed
  variant1   the finding of DESIGN.md section 2.8: how often the appended variant is strictly better (ADD, SCA) than
             the incumbent (:613) or than variant 0 of the same seed, over every candidate above

Run from the repository root: python tests/golden/make_lin_costs.py  (about two minutes on 8 cores)."""
import glob
import json
import os
import sys
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import lin_oracle as O  # noqa: E402
from plo_testlib import DATA, read_sms  # noqa: E402

SEEDS = list(range(8))
LONG_NAME, LONG = "4x4x4_49_156_L", 10000


def fixtures():
    out = []
    for f in sorted(glob.glob(os.path.join(DATA, "*.sms"))):
        try:
            read_sms(f)
        except ValueError:                     # symbolic placeholders (-X_): not rational
            continue
        out.append(os.path.basename(f)[:-4])
    return out


def rows_for(name, tr):
    m, n, e = read_sms(os.path.join(DATA, name + ".sms"))
    if tr:
        m, n, e = O.transpose(m, n, e)
    return O.rows_of(m, n, e), n


def job(arg):
    name, tr, seeds = arg
    rows, n = rows_for(name, tr)
    return [O.cost6(rows, n, s) for s in seeds]


def main():
    names = fixtures()
    jobs = [(nm, tr, [O.BASE_SEED] + SEEDS) for nm in names for tr in (False, True)]
    chunks = [(LONG_NAME, False, list(range(s, min(s + 250, LONG)))) for s in range(0, LONG, 250)]
    with Pool() as p:
        res = p.map(job, jobs + chunks, chunksize=1)
    fx = {}
    v1_base = v1_v0 = total = 0
    for (nm, tr, _), r in zip(jobs, res):
        fx[nm + ("|t" if tr else "|d")] = r
        base = r[0]
        for c in r[1:]:
            total += 1
            v1_base += O.better(c[3:6], base[:3])
            v1_v0 += O.better(c[3:6], c[:3])
    long_ops = [x for r in res[len(jobs):] for c in r for x in c]
    lbase = job((LONG_NAME, False, [O.BASE_SEED]))[0]
    lv1 = sum(O.better(long_ops[6 * k + 3:6 * k + 6], lbase[:3]) for k in range(LONG))
    lv1v0 = sum(O.better(long_ops[6 * k + 3:6 * k + 6], long_ops[6 * k:6 * k + 3]) for k in range(LONG))
    lmin = min((long_ops[6 * k + 3], long_ops[6 * k + 4]) for k in range(LONG))
    out = {
        "stream": "include/plinopt_hip.h CandRng; Fisher-Yates over the rows, then the draws of variant 0, then of variant 1",
        "base_seed": O.BASE_SEED, "seeds": SEEDS,
        "fixtures": fx,
        "long": {"name": LONG_NAME, "seed0": 0, "n": LONG, "base": lbase, "ops": long_ops},
        "variant1": {"fixture_candidates": total, "beats_incumbent": v1_base, "beats_variant0": v1_v0,
                     "long_beats_incumbent": lv1, "long_beats_variant0": lv1v0, "long_min_add_sca": list(lmin)},
    }
    with open(os.path.join(HERE, "lin_costs.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(json.dumps(out["variant1"]))


if __name__ == "__main__":
    main()
