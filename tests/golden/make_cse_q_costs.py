"""Writes tests/golden/cse_q_costs.json: per case of tests/cse_q_cases.py that runs, (adds, muls) of Optimizer() over Q for the
seeds 0 .. nseeds-1, from the Python restatement tests/cse_q_oracle.py (exact fractions; no product code): 256 seeds for the small
cases, 150 for 4x4x4_48_rational_L, 64 for the other fixtures.  Takes a few minutes on 8 processes.

Run from the repository root: python tests/golden/make_cse_q_costs.py"""
import json
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import cse_q_cases  # noqa: E402
import cse_q_oracle as O  # noqa: E402


def score(job):
    c, s0, s1 = job
    rows = O.field_rows(O.QQ(), c.m, c.ent)
    return c.name, s0, [O.Optimizer(O.QQ(), rows, c.n, s).run() for s in range(s0, s1)]


def main():
    cases = cse_q_cases.running()
    jobs = [(c, s0, min(s0 + 16, c.nseeds)) for c in cases for s0 in range(0, c.nseeds, 16)]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        parts = sorted(pool.map(score, jobs, chunksize=1), key=lambda r: (r[0], r[1]))
    costs = {c.name: [] for c in cases}
    for name, _, part in parts:
        costs[name] += part
    lines = [json.dumps({"name": c.name, "adds": [a for a, _ in costs[c.name]], "muls": [m for _, m in costs[c.name]]}) for c in cases]
    with open(os.path.join(HERE, "cse_q_costs.json"), "w") as f:
        f.write("{\"cases\": [\n" + ",\n".join(lines) + "\n]}\n")
    print(len(cases), "cases,", sum(len(v) for v in costs.values()), "candidates")


if __name__ == "__main__":
    main()
