"""Writes tests/golden/kmethod_synth_costs.json: per restart (adds, muls, rank, NotIndep, dependent rows computed through
Dep) of the kernel method (bin/optimizer -K, reference include/plinopt_optimize.inl:1299-1340 with this build's
decomposition rule) on the synthetic edge cases of tests/synth.py (kmethod_cases), computed by the C oracle
(oracle/plo_oracle.c plo_oracle_kernel_restart).

  cases      one entry per case: name, family, the SHA-256 of its text (synth.km_text; no matrix is stored, they are
             regenerated), the modulus, "runs" (plo_kernel_search takes a seed range only: every case is scored as the
             (seed0, n) runs of synth.SEED_RUNS with per_block = 1), its seeds and the oracle's five counts per seed.
             Every admitted case is "quick": tests/test_synth_golden.py recomputes all of them.  A case the device
             refuses holds the name of the header's code and nothing else.
  per_block  the restarts of the first seeds of the blocks of synth.KM_PER_BLOCK (seed0, restarts, per_block) on
             km_a_64x32_vals: a block shares the decomposition of its first seed

Run from the repository root: python tests/golden/make_kmethod_synth_costs.py  (1 s: the oracle takes 25 ms for
the eleven restarts of 128x64 and 0.23 s for those of km_c_64x16_dense; the times are printed, not stored)."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import synth  # noqa: E402
from plo_testlib import OracleMatrix  # noqa: E402

PER_BLOCK_CASE = "km_a_64x32_vals"


def oracle_matrix(c):
    return OracleMatrix(*c.csr, c.p)


def main():
    t0 = time.time()
    cases = synth.kmethod_cases()
    out_cases = []
    for c in cases:
        e = {"name": c.name, "family": c.family, "sha256": c.sha256}
        if c.refusal:
            e["refusal"] = c.refusal
        else:
            t1 = time.time()
            M = oracle_matrix(c)
            ops = [list(M.kernel_restart(s)) for s in c.seeds]
            print("%-24s %3d x %2d mod %10d rank %2d  %6.3f s" % (c.name, c.m, c.n, c.p, c.rank, time.time() - t1))
            e.update(p=c.p, mode=c.mode, seeds=c.seeds, quick=c.quick, out=ops)
        out_cases.append(e)
    s0, n, per = synth.KM_PER_BLOCK
    M = oracle_matrix(next(c for c in cases if c.name == PER_BLOCK_CASE))
    firsts = list(range(s0, s0 + n, per))
    per_block = {"name": PER_BLOCK_CASE, "seed0": s0, "n": n, "per_block": per, "seeds": firsts, "out": [list(M.kernel_restart(s)) for s in firsts]}
    out = {"oracle": "oracle/plo_oracle.c plo_oracle_kernel_restart on tests/synth.py kmethod_cases", "seed_runs": [list(r) for r in synth.SEED_RUNS],
           "cases": out_cases, "per_block": per_block}
    with open(os.path.join(HERE, "kmethod_synth_costs.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("%d cases (%d refusals); total %.0f s" % (len(cases), sum(1 for c in cases if c.refusal), time.time() - t0))


if __name__ == "__main__":
    main()
