"""Writes tests/golden/orbit_cse_cases.json: name -> sha256 of synth.orbit_text of every case of tests/orbit_cse_cases.py, so that a
change of the generator shows up in tests/test_orbit_cse_cases_host.py.  Run from the repository root: python tests/golden/make_orbit_cse_cases.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import orbit_cse_cases as cc  # noqa: E402

if __name__ == "__main__":
    pins = {c.name: c.sha256 for p in cc.PRIMES for c in cc.all_cases(p)}
    with open(os.path.join(HERE, "orbit_cse_cases.json"), "w") as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(pins), "cases")
