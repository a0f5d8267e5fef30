"""Writes tests/golden/orbit_growth_costs.json: (bits of the cost, nnz, nno) per seed of the growth-factor measure, scored by the
literal oracle tests/orbit_growth_oracle.py, for the inputs of tests/orbit_growth_cases.py:
  fixtures  the four fixture triples, both actions, SEEDS
  cases     the synthetic edge shapes, both actions, SEEDS (or the code of the refusal, scored all the same: the host takes them)
  bound     the triples one step inside and outside the 2^53 proof, SEEDS
  synth     the triples over Q of synth.orbit_cases() (each once: the canonical family repeats them), both actions, HOST_SEEDS
  search    the argmin under (bits, nnz, nno, seed) over seeds 0 .. SEARCH_N - 1 and how many seeds share its (bits, nnz, nno)
The costs are stored as 16 hex digits: the pattern of the double.  Run from the repository root:
  python tests/golden/make_orbit_growth_costs.py [processes]
tests/test_synth_golden.py's rule applies: the file is reproduced byte for byte, and tests/test_orbiter_growth_host.py recomputes
the entries the oracle scores quickly."""
import json
import os
import sys
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import orbit_growth_cases as C  # noqa: E402
import orbit_growth_oracle as G  # noqa: E402
import orbit_oracle as O  # noqa: E402
import synth  # noqa: E402
from plo_testlib import DATA  # noqa: E402


def case_mats(c):
    return [O.dense(*M) for M in (c.L, c.R, c.P)], c.mkn


def synth_cases():
    """the triples over Q of synth.orbit_cases(), each once"""
    seen, out = set(), []
    for c in synth.orbit_cases():
        text = "".join(synth.sms_text(*M) for M in (c.L, c.R, c.P))
        if c.modulus == 0 and text not in seen:
            seen.add(text)
            out.append(c)
    return out


_INPUTS = {}


def inputs(kind, name):
    if (kind, name) not in _INPUTS:
        if kind == "fixture":
            _INPUTS[kind, name] = O.load(os.path.join(DATA, name))
        else:
            pool = {"case": C.cases, "bound": lambda: [c for c, _, _ in C.bound_cases()], "synth": synth_cases}[kind]()
            _INPUTS[kind, name] = case_mats({c.name: c for c in pool}[name])
    return _INPUTS[kind, name]


def score(task):
    kind, name, action, seeds = task
    mats, mkn = inputs(kind, name)
    return [["%016x" % G.bits(c[0]), c[1], c[2]] for c in (G.cost3(mats, mkn, s, action) for s in seeds)]


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    jobs = []                                              # (slot in the document, task)
    doc = {"seeds": C.SEEDS, "host_seeds": C.HOST_SEEDS, "fixtures": [], "cases": [], "bound": [], "synth": [], "search": []}

    def add(entry, field, kind, name, action, seeds, chunk=8):
        entry[field] = []
        for i in range(0, len(seeds), chunk):
            jobs.append((entry, field, (kind, name, action, seeds[i:i + chunk])))

    for name in C.FIXTURES:
        e = {"name": name, "out": {}}
        for a, an in C.ACTION_NAMES.items():
            add(e["out"], an, "fixture", name, a, C.SEEDS)
        doc["fixtures"].append(e)
    for c in C.cases():
        e = {"name": c.name, "sha256": c.sha256, "refusal": {an: C.growth_refusal(c, a) for a, an in C.ACTION_NAMES.items()}, "out": {}}
        for a, an in C.ACTION_NAMES.items():
            add(e["out"], an, "case", c.name, a, C.SEEDS)
        doc["cases"].append(e)
    for c, a, refused in C.bound_cases():
        e = {"name": c.name, "sha256": c.sha256, "action": C.ACTION_NAMES[a], "refused": refused}
        add(e, "out", "bound", c.name, a, C.SEEDS)
        doc["bound"].append(e)
    for c in synth_cases():
        e = {"name": c.name, "sha256": c.sha256, "quick": c.quick, "out": {}}
        for a, an in C.ACTION_NAMES.items():
            add(e["out"], an, "synth", c.name, a, C.HOST_SEEDS, chunk=2)
        doc["synth"].append(e)
    searches = []
    for name in C.SEARCH_FIXTURES:
        for a, an in C.ACTION_NAMES.items():
            e = {"name": name, "action": an, "seed0": 0, "n": C.SEARCH_N}
            add(e, "all", "fixture", name, a, list(range(C.SEARCH_N)), chunk=64)
            searches.append(e)
    with Pool(procs) as pool:
        for (entry, field, _), res in zip(jobs, pool.imap(score, [t for _, _, t in jobs], chunksize=1)):
            entry[field] += res
    for e in searches:
        allc = e.pop("all")
        best = min((int(b, 16), nnz, nno, s) for s, (b, nnz, nno) in enumerate(allc))
        e["best"] = ["%016x" % best[0], best[1], best[2], best[3]]
        e["tied"] = sum(1 for b, nnz, nno in allc if (int(b, 16), nnz, nno) == best[:3])
        e["tied_cost"] = sum(1 for b, _, _ in allc if int(b, 16) == best[0])
        doc["search"].append(e)
    with open(os.path.join(HERE, "orbit_growth_costs.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
