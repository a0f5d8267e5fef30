"""Writes tests/golden/lin_synth_costs.json: the per-seed (ADD, SCA, ROWS) of variant 0 and of variant 1 of the in-place
linear search (bin/inplacer, reference include/plinopt_inplace.inl:604-673) on the synthetic edge cases of
tests/synth.py (lin_cases, lin_tie_cases), computed by the literal oracle tests/lin_oracle.py.

  cases   one entry per case: name, family, the SHA-256 of its text (synth.sms_text; no matrix is stored, they are
          regenerated), how it is scored ("list": one explicit seed list, "runs": the (seed0, n) runs of synth.SEED_RUNS),
          its seeds and the oracle's cost6 per seed.  "quick" marks the cases tests/test_synth_golden.py recomputes: those
          that take under a second of oracle time, by a fixed rule on the case's size (synth.lin_quick) and not by the
          measured time, so that this file is reproduced byte for byte.  A case the device refuses holds the name of the header's code and nothing else.
  tie     three tiny matrices, seeds TIE_SEED0 .. TIE_SEED0 + TIE_N - 1 flattened 6 per seed, the incumbent (BASE_SEED)
          and the result of lin_oracle.search: the argmin under (ADD, SCA, seed, variant) and the incumbent rule

Run from the repository root: python tests/golden/make_lin_synth_costs.py  (42 s with 8 workers on 8 cores, all busy;
the longest cases, lin_h_unit and lin_i_rat, take 38-39 s of oracle time each in that pool and about half of that on an
idle machine, lin_c_four_unit and lin_c_ones 22 s; the times are printed, not stored)."""
import json
import os
import sys
import time
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import lin_oracle as O  # noqa: E402
import synth  # noqa: E402


def rows_of(c):
    return O.rows_of(c.m, c.n, c.ent)


def job(arg):
    kind, idx, seeds = arg
    c = (synth.lin_cases() if kind == "case" else synth.lin_tie_cases())[idx]
    rows = rows_of(c)
    t0 = time.time()
    return [O.cost6(rows, c.n, s) for s in seeds], time.time() - t0


def main():
    t0 = time.time()
    cases, ties = synth.lin_cases(), synth.lin_tie_cases()
    jobs = [("case", i, c.seeds) for i, c in enumerate(cases) if not c.refusal]
    jobs.sort(key=lambda j: -(4 * cases[j[1]].nnz + 3 * cases[j[1]].m))          # the long ones first
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
            ops, secs = got[c.name]
            print("%-28s m %5d nnz %5d waves %d  %6.2f s%s" % (c.name, c.m, c.nnz, c.waves, secs, "  (quick)" if c.quick else ""))
            if c.quick and secs >= 1.0:
                print("  note: a quick case took a second or more here")
            e.update(mode=c.mode, seeds=c.seeds, quick=c.quick, out=ops)
        out_cases.append(e)
    out_ties = []
    for i, c in enumerate(ties):
        ops = [x for (_, j, _), (r, _) in zip(chunks, res[len(jobs):]) if j == i for c6 in r for x in c6]
        rows = rows_of(c)
        best, seed, var = O.search(rows, c.n, synth.TIE_SEED0, synth.TIE_N)
        out_ties.append({"name": c.name, "sha256": c.sha256, "seed0": synth.TIE_SEED0, "n": synth.TIE_N, "base": O.cost6(rows, c.n, O.BASE_SEED),
                         "out": ops, "search": [list(best), seed, var]})
    out = {"oracle": "tests/lin_oracle.py cost6 on tests/synth.py lin_cases / lin_tie_cases", "base_seed": O.BASE_SEED,
           "seed_runs": [list(r) for r in synth.SEED_RUNS], "cases": out_cases, "tie": out_ties}
    with open(os.path.join(HERE, "lin_synth_costs.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("%d cases (%d refusals), %d tie cases; total %.0f s" % (len(cases), sum(1 for c in cases if c.refusal), len(ties), time.time() - t0))


if __name__ == "__main__":
    main()
