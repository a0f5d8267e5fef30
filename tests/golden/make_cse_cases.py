"""Writes tests/golden/cse_cases.json: the edge cases of the one-wave CSE kernel (tests/synth.py cse_cases) by name, family,
shape, modulus, entries and the SHA-256 of their text (synth.km_text; no matrix is stored, they are regenerated), with the slots
of the first pair table as synth.wave_plan sizes it, or the name of the header's code for a matrix that goes to the HBM family.
No costs: the C oracle scores every case live, in under two seconds for the whole list (tests/test_cse_cases_host.py prints the
time).  tests/test_synth_golden.py holds the generators to this file.

Run from the repository root: python tests/golden/make_cse_cases.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import synth  # noqa: E402


def entry(c):
    e = {"name": c.name, "family": c.family, "m": c.m, "n": c.n, "p": c.p, "nnz": len(c.csr[3]), "sha256": c.sha256}
    if c.hbm:
        e["refusal"] = c.plan
    else:
        e["cap"] = c.plan.cap
    return e


def main():
    out = {"cases": [entry(c) for c in synth.cse_cases()]}
    with open(os.path.join(HERE, "cse_cases.json"), "w") as f:
        f.write("{\"cases\": [\n" + ",\n".join(json.dumps(e) for e in out["cases"]) + "\n]}\n")
    print(len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
