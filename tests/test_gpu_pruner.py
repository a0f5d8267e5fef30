"""bin/pruner --gpu 1 (all windows of a method in one plo_cse_batch_search call) prints what --gpu 0 prints, byte for byte."""
import os

import pytest

import pruner_lib as pl
from plo_testlib import DATA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _build():
    pl.build()


def both(args):
    rc1, out1, err1 = pl.run(args + ["--gpu", "1"])
    rc0, out0, err0 = pl.run(args + ["--gpu", "0"])
    assert rc1 == 0 and rc0 == 0, (err1, err0)
    assert out1 == out0 and out1
    assert "# GPU: " in err1 and "# GPU: " not in err0
    return out1, err1


def test_all_pairs_of_3x4x7():
    out, err = both(["-q", 131071, "-O", 50, os.path.join(DATA, "3x4x7_63_rational_R.slp")])
    assert len(pl.report(out)) == 225
    for method in ("-D", "-G"):
        calls = [l for l in err.splitlines() if "plo_cse_batch_search" in l and "# GPU: " + method + " " in l]
        assert len(calls) == 1 and "over 225 windows" in calls[0], err


def test_singles_of_4x4x4_with_a_31_bit_prime():
    out, err = both(["-q", 2147483629, "-v", "-O", 50, os.path.join(DATA, "4x4x4_49_156_P.slp")])
    assert len(pl.report(out)) == 19


def test_apply_on_the_planted_fixture():
    out, err = both(["-q", 131071, "-O", 10, "--apply", os.path.join(DATA, "pruner_planted.slp")])
    assert "--apply: window" in err and ":=" in out
