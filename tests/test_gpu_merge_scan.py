"""The scan and the prefetch of the merge's sum pass (plo::defer_merge, pass B) against the LITERAL oracle.

Pass B sums a group of partitions in an LDS table of 2^lb slots, lb = 6..13 by the group's records.  A thread
  * puts its six prefetched records (tid + k nth of the group, k < 6; 3072 in all) into the table; records behind 3072
    (`merge_loop_records`) are loaded inside the group, six at a time;
  * reads its slots tid + u nth of the table up front, empties the ones that held a key of frequency below 2, keeps a bit per
    live one and writes back one triple per set bit, emptying that slot.

What can go wrong, and the case that reaches it (the knobs are those of tests/test_gpu_merge_groups.py, whose docstring gives the
bounds on the counters; both literal-oracle fixtures, every case bit for bit with no repeat on the eager table):

  natural run, PLO_BIG_LGRP=64        groups of one partition, tables of 2^9 .. 2^13 slots: threads with 1 to 16 slots, the second
                                      batch of eight reads taken (2^13) and skipped
  PLO_BIG_LOGTRIG=2000 (+ HWIN=64)    dozens of merges per candidate; the late ones sum near-empty partitions in groups of up to
                                      64 (sh.outcnt[j], j up to 63) and tables of 2^8 slots: fewer slots than threads, so whole
                                      waves own no slot and must still reach both barriers; groups that write back nothing
    ... + PLO_BIG_LGRP=64             the same merges in groups of at most 64 records: tables of 2^6 and 2^7 slots
  PLO_BIG_LGRP=3072, 3073, 7000       a group exactly at the prefetch, one record past it, and the loop behind it (2^13 slots)
  PLO_BIG_WIDE=1                      the instances with 64-bit offsets share the code

One case per group runs in a child process with PLO_BIG_STATS=1 and reads the OR of the launch's table sizes from the library's
stderr line: TABLES says which sizes a case must have reached, with the reason.  The sizes follow from lb's rule (the smallest
2^lb >= 2 tot + 64, tot the group's records): 2^13 needs a group of more than 2016 records, 2^6 or 2^7 one of at most 32.
"""
import json
import os
import re
import subprocess
import sys

import pytest

if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from plo_testlib import GOLDEN, l32_cut, l32_rows, longrow_matrix

pytestmark = pytest.mark.gpu
P = 131071
KNOBS = ("PLO_BIG_LGRP", "PLO_BIG_LOGTRIG", "PLO_BIG_HWIN", "PLO_BIG_WIDE")

NATURAL = {}
SINGLE = {"PLO_BIG_LGRP": "64"}
FORCED = {"PLO_BIG_LOGTRIG": "2000"}
FORCED_SMALL_WINDOW = {"PLO_BIG_LOGTRIG": "2000", "PLO_BIG_HWIN": "64"}
FORCED_SMALL_GROUPS = {"PLO_BIG_LOGTRIG": "2000", "PLO_BIG_HWIN": "64", "PLO_BIG_LGRP": "64"}
AT_PREFETCH = {"PLO_BIG_LGRP": "3072"}
PAST_PREFETCH = {"PLO_BIG_LGRP": "3073"}
LOOP = {"PLO_BIG_LGRP": "7000"}
WIDE = {"PLO_BIG_WIDE": "1"}
CASES = [NATURAL, SINGLE, FORCED, FORCED_SMALL_WINDOW, FORCED_SMALL_GROUPS, AT_PREFETCH, PAST_PREFETCH, LOOP]


def _id(env):
    return "+".join("%s=%s" % (k[8:].lower(), v) for k, v in sorted(env.items())) or "natural"


def _fixture(name):
    """(csr, (adds, muls)) of a literal-oracle fixture: the 128-row cut with seeds 1..8, the long rows with seeds 1..4"""
    if name == "cut":
        G = json.load(open(os.path.join(GOLDEN, "l32cut_costs.json")))
        _, _, rows = l32_rows(P)
        csr = l32_cut(G["row_lo"], G["row_hi"], P, rows)
        want = (G["adds"][:8], G["muls"][:8])
    else:
        G = json.load(open(os.path.join(GOLDEN, "longrow_costs.json")))
        csr = longrow_matrix(P)
        want = (G["adds"], G["muls"])
    assert len(csr[3]) == G["nnz"] and G["seed0"] == 1
    return csr, want


def _run(csr, n, env):
    """costs and counters of seeds 1 .. n with the knobs of `env` set (the plan reads them when it is built)"""
    from plinopt_amd import CSEPlan
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(env)
        m, nn, rp, c, v = csr
        plan = CSEPlan(m, nn, rp, c, v, P)
        assert plan.is_hbm
        got = plan.cost_many(seed0=1, n=n)
        cnt = plan.hbm_counters()
        plan.close()
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    print("HBM counters %s: %s" % (_id(env), cnt))
    return got, cnt


@pytest.fixture(scope="module")
def cut(hip):
    return _fixture("cut")


@pytest.fixture(scope="module")
def longrow(hip):
    return _fixture("longrow")


def _check(fx, env):
    csr, want = fx
    got, cnt = _run(csr, len(want[0]), env)
    assert got == want
    assert cnt["candidates"] == len(want[0]) and cnt["eager_refits"] == 0, cnt
    if "PLO_BIG_LOGTRIG" in env:
        assert cnt["forced_merges"] >= 10 * len(want[0]), cnt             # (the bound of test_gpu_merge_groups: 10^5 log records per candidate)
    if env.get("PLO_BIG_LGRP") == "7000":
        assert cnt["merge_loop_records"] > 0, cnt
    if "PLO_BIG_LGRP" not in env:
        assert cnt["merge_loop_records"] == 0, cnt                        # the default plan's groups (up to 3000 records) are prefetched whole
    return cnt


@pytest.mark.parametrize("env", CASES, ids=_id)
def test_cut(cut, env):
    _check(cut, env)


@pytest.mark.parametrize("env", CASES, ids=_id)
def test_longrow(longrow, env):
    _check(longrow, env)


def test_cut_wide_offsets_beyond_the_prefetch(cut):
    _check(cut, dict(WIDE, **LOOP))


# (fixture, knobs) -> (sizes 2^lb of which AT LEAST ONE must have been reached, sizes that must ALL have been reached, why)
# The masks of one run, in this order: 0x3d00, 0x3f00, 0x0f80, 0x3000, 0x3800.
TABLES = [
    ("longrow", SINGLE, 0x1E00, 0, "single partitions of a few hundred to a few thousand records: 2^9 .. 2^12"),
    ("cut", FORCED_SMALL_WINDOW, 0, 0x0100, "late forced merges: 64 near-empty partitions to a group, 33 .. 96 records (2^6 and 2^7 are out of this "
                                           "case's reach: a group ends at 64 partitions or 3000 records, and 64 partitions hold more than 32)"),
    ("cut", FORCED_SMALL_GROUPS, 0x00C0, 0, "the same merges in groups of at most 64 records: the late ones hold at most 32"),
    ("cut", LOOP, 0, 0x2000, "groups of up to 7000 records: above 2016, the whole table"),
    ("longrow", dict(WIDE, **AT_PREFETCH), 0, 0x2000, "groups of up to 3072 records: above 2016, the whole table"),
]


def _child(name, env):
    """the case in a process of its own with PLO_BIG_STATS=1: (costs, counters, OR of the table sizes)"""
    cenv = {k: v for k, v in os.environ.items() if k not in KNOBS}
    cenv.update(env, PLO_BIG_STATS="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, json.dumps(env)], capture_output=True, text=True, env=cenv, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.splitlines()[-1])
    masks = [int(x, 16) for x in re.findall(r"summing-table sizes of the launch's groups \(OR of 1 << lb\): 0x([0-9a-f]+)", r.stderr)]
    assert masks, r.stderr
    mask = 0
    for x in masks:
        mask |= x
    print("table sizes %s %s: 0x%x" % (name, _id(env), mask))
    return out, mask


@pytest.mark.parametrize("name,env,any_of,all_of,why", TABLES, ids=["%s-%s" % (t[0], _id(t[1])) for t in TABLES])
def test_table_sizes_reached(hip, name, env, any_of, all_of, why):
    out, mask = _child(name, env)
    assert out["ok"] and out["counters"]["eager_refits"] == 0, out
    assert mask & ~0x3FC0 == 0, hex(mask)                                 # lb = 6 .. 13
    assert (not any_of or mask & any_of) and mask & all_of == all_of, (hex(mask), why)


if __name__ == "__main__":
    from plinopt_amd import capi
    capi.check(capi.lib().plo_init(0))
    fx = _fixture(sys.argv[1])
    got, cnt = _run(fx[0], len(fx[1][0]), json.loads(sys.argv[2]))
    print(json.dumps({"ok": [list(got[0]), list(got[1])] == [list(fx[1][0]), list(fx[1][1])], "counters": cnt}))
