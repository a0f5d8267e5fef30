"""Writes tests/golden/tril_synth_costs.json: the per-seed (ADD, SCA, MUL) of the oriented and of the unoriented program
of the in-place trilinear search (bin/trilplacer, reference include/plinopt_inplace.inl:812-929; `-e`: :507-598) on the
synthetic edge cases of tests/synth.py (tril_cases, tril_tie_cases), computed by the C oracle (oracle/plo_tril_oracle.c).

  cases   one entry per case: name, family, the SHA-256 of its text (synth.tril_text; no matrix is stored, they are
          regenerated), expanded (`-e`), how it is scored ("list": one explicit seed list, "runs": the (seed0, n) runs of
          synth.SEED_RUNS), its seeds and the oracle's six counts per seed.  "quick" marks the cases
          tests/test_synth_golden.py recomputes, by a fixed rule on the case's size (synth.tril_quick) and not by the
          measured time, so that this file is reproduced byte for byte.  The two programs near the 160 KiB of LDS have
          three seeds.  A case the device refuses holds the name of the header's code and nothing else.
  tie     two tiny triples, seeds TIE_SEED0 .. TIE_SEED0 + TRIL_TIE_N - 1 flattened 6 per seed, and the oracle's search:
          the argmin under (ADD, SCA, seed, variant)

Run from the repository root: python tests/golden/make_tril_synth_costs.py  (23 s with 8 workers: the three seeds of
tril_e_600x200_rat_e take 11 s of oracle time, those of tril_e_1200x200_unit and the eleven of tril_e_200x64_rat_e 1 s each;
the times are printed, not stored)."""
import json
import os
import sys
import time
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import synth  # noqa: E402
from plo_testlib import OracleTril  # noqa: E402


def oracle_tril(c):
    (na, A), (nb, B), (nt, T) = c.mats
    return OracleTril((c.m, na, A), (c.m, nb, B), (nt, c.m, {(j, i): v for (i, j), v in T.items()}))


def job(idx):
    c = synth.tril_cases()[idx]
    t0 = time.time()
    ops = oracle_tril(c).cost_many(seeds=c.seeds, expanded=c.expanded)
    return [list(a) + list(b) for a, b in ops], time.time() - t0


def main():
    t0 = time.time()
    cases, ties = synth.tril_cases(), synth.tril_tie_cases()
    jobs = [i for i, c in enumerate(cases) if not c.refusal]
    jobs.sort(key=lambda i: -cases[i].cap * len(cases[i].seeds))                 # the long ones first
    with Pool(min(8, os.cpu_count() or 1)) as p:
        res = p.map(job, jobs, chunksize=1)
    got = {cases[i].name: r for i, r in zip(jobs, res)}
    out_cases = []
    for c in cases:
        e = {"name": c.name, "family": c.family, "sha256": c.sha256}
        if c.refusal:
            e["refusal"] = c.refusal
        else:
            ops, secs = got[c.name]
            print("%-28s m %5d cap %5d waves %d lds %6d  %6.2f s%s" % (c.name, c.m, c.cap, c.waves, c.lds, secs, "  (quick)" if c.quick else ""))
            if c.quick and secs >= 1.0:
                print("  note: a quick case took a second or more here")
            e.update(expanded=c.expanded, mode=c.mode, seeds=c.seeds, quick=c.quick, out=ops)
        out_cases.append(e)
    out_ties = []
    for c in ties:
        O = oracle_tril(c)
        ops = [x for a, b in O.cost_many(seed0=synth.TIE_SEED0, nseeds=synth.TRIL_TIE_N, expanded=c.expanded) for x in list(a) + list(b)]
        best, seed, var = O.search(synth.TIE_SEED0, synth.TRIL_TIE_N, expanded=c.expanded)
        out_ties.append({"name": c.name, "sha256": c.sha256, "expanded": c.expanded, "seed0": synth.TIE_SEED0, "n": synth.TRIL_TIE_N, "out": ops,
                         "search": [list(best), seed, var]})
    out = {"oracle": "oracle/plo_tril_oracle.c plo_oracle_tril_cost_many_x on tests/synth.py tril_cases / tril_tie_cases", "base_seed": synth.BASE_SEED,
           "seed_runs": [list(r) for r in synth.SEED_RUNS], "cases": out_cases, "tie": out_ties}
    with open(os.path.join(HERE, "tril_synth_costs.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("%d cases (%d refusals), %d tie cases; total %.0f s" % (len(cases), sum(1 for c in cases if c.refusal), len(ties), time.time() - t0))


if __name__ == "__main__":
    main()
