"""Writes tests/golden/orbit_synth_costs.json: the per-seed (cost, nnz, nno) of the De Groote orbit search (bin/orbiter,
reference src/orbiter.cpp:272-324) on the synthetic edge cases of tests/synth.py (orbit_cases, orbit_tie_cases), computed by
the literal oracle tests/orbit_oracle.py with the case's modulus and measure (under a modulus the oracle scores by density
whatever the measure: family f).

  cases   one entry per case: name, family, the SHA-256 of its text (synth.orbit_text; no matrix is stored, they are
          regenerated), modulus, measure, how it is scored ("list": one explicit seed list, "runs": the (seed0, n) runs of
          synth.SEED_RUNS), its seeds and the oracle's cost3 per seed.  "quick" marks the cases tests/test_synth_golden.py
          recomputes: those that take under a second of oracle time, by a fixed rule on the case's size (synth.orbit_quick)
          and not by the measured time, so that this file is reproduced byte for byte.  A case the device refuses holds the name of the header's code and nothing else.
  tie     three tiny triples, seeds TIE_SEED0 .. TIE_SEED0 + TIE_N - 1 flattened 3 per seed, and the input's own counts

Run from the repository root: python tests/golden/make_orbit_synth_costs.py  (22 s with 8 workers on 8 cores, all busy; the
longest case, the 16x16x16 triple modulo 3, takes 15 s of oracle time in that pool; the times are printed, not stored)."""
import json
import os
import sys
import time
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import orbit_oracle as O  # noqa: E402
import synth  # noqa: E402


def mats_of(c):
    mats = [O.dense(*M) for M in (c.L, c.R, c.P)]
    return [M if O.small_ints(M) is None else O.small_ints(M) for M in mats]


def job(arg):
    kind, idx, seeds = arg
    c = (synth.orbit_cases() if kind == "case" else synth.orbit_tie_cases())[idx]
    mats = mats_of(c)
    t0 = time.time()
    return [list(O.cost3(mats, c.mkn, s, modulus=c.modulus, measure=c.measure)) for s in seeds], time.time() - t0


def main():
    t0 = time.time()
    cases, ties = synth.orbit_cases(), synth.orbit_tie_cases()
    jobs = [("case", i, c.seeds) for i, c in enumerate(cases) if not c.refusal]
    jobs.sort(key=lambda j: -cases[j[1]].r * sum(cases[j[1]].mkn) * (1 if cases[j[1]].quick else 50))      # the long ones first
    chunks = [("tie", i, list(range(s, min(s + 250, synth.TIE_SEED0 + synth.TIE_N)))) for i in range(len(ties))
              for s in range(synth.TIE_SEED0, synth.TIE_SEED0 + synth.TIE_N, 250)]
    with Pool(min(8, os.cpu_count() or 1)) as p:
        res = p.map(job, jobs + chunks, chunksize=1)
    got = {cases[i].name: r for (_, i, _), r in zip(jobs, res)}
    out_cases = []
    for c in cases:
        e = {"name": c.name, "family": c.family, "sha256": c.sha256}
        if c.refusal:
            e["refusal"] = c.refusal
        else:
            out3, secs = got[c.name]
            print("%-36s %2dx%2dx%2d r %4d nnz %5d waves %d  %6.2f s%s" % ((c.name,) + c.mkn + (c.r, c.nnz, c.waves, secs, "  (quick)" if c.quick else "")))
            if c.quick and secs >= 1.0:
                print("  note: a quick case took a second or more here")
            e.update(modulus=c.modulus, measure=c.measure, mode=c.mode, seeds=c.seeds, quick=c.quick, out=out3)
        out_cases.append(e)
    out_ties = []
    for i, c in enumerate(ties):
        out3 = [x for (_, j, _), (r, _) in zip(chunks, res[len(jobs):]) if j == i for c3 in r for x in c3]
        out_ties.append({"name": c.name, "sha256": c.sha256, "modulus": c.modulus, "measure": c.measure, "seed0": synth.TIE_SEED0, "n": synth.TIE_N,
                         "base": list(O.cost3(mats_of(c), c.mkn, O.BASE_SEED, modulus=c.modulus, measure=c.measure)), "out": out3})
    out = {"oracle": "tests/orbit_oracle.py cost3 on tests/synth.py orbit_cases / orbit_tie_cases", "base_seed": O.BASE_SEED,
           "seed_runs": [list(r) for r in synth.SEED_RUNS], "cases": out_cases, "tie": out_ties}
    with open(os.path.join(HERE, "orbit_synth_costs.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("%d cases (%d refusals), %d tie cases; total %.0f s" % (len(cases), sum(1 for c in cases if c.refusal), len(ties), time.time() - t0))


if __name__ == "__main__":
    main()
