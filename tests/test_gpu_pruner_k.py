"""bin/pruner -K --gpu 1 (the windows that have a kernel in one plo_kernel_batch_search call) prints what --gpu 0 prints,
byte for byte, and the device refuses none of these small windows."""
import os

import pytest

import pruner_k_lib as kl
from plo_testlib import DATA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _build():
    kl.pl.build()


def both(args):
    rc1, out1, err1 = kl.run(args + ["--gpu", "1"])
    rc0, out0, err0 = kl.run(args + ["--gpu", "0"])
    assert rc1 == 0 and rc0 == 0, (err1, err0)
    assert out1 == out0 and out1
    assert "# GPU: " in err1 and "# GPU: " not in err0
    assert "# refused:" not in err1, err1
    return out1, err1


@pytest.mark.parametrize("letter,nwin,nk", [("L", 100, 100), ("R", 225, 118)])
def test_all_pairs_of_3x4x7(letter, nwin, nk):
    out, err = both(["-q", 131071, "-K", "-O", 50, os.path.join(DATA, "3x4x7_63_rational_%s.slp" % letter)])
    got = kl.report(out)
    assert len(got) == nwin and sum(1 for g in got if g["K"]) == nk
    calls = [l for l in err.splitlines() if "plo_kernel_batch_search" in l]
    assert len(calls) == 1 and "# GPU: -K one plo_kernel_batch_search call over %d windows" % nk in calls[0], err
    assert "plo_cse_batch_search" not in err


def test_all_methods_and_apply_on_the_planted_fixture():
    out, err = both(["-q", 131071, "-O", 10, "-D", "-K", "-G", "--apply", os.path.join(DATA, "pruner_planted.slp")])
    assert "--apply: window" in err and ":=" in out
    assert sum(1 for l in err.splitlines() if "plo_kernel_batch_search" in l) == 1 and sum(1 for l in err.splitlines() if "plo_cse_batch_search" in l) == 2
