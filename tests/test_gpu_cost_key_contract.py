"""The cost key of every CSE search entry point, pinned against the entry's own per-candidate outputs.

A search packs (cost key, seed offset) into one word per candidate, takes the minimum on the device and decodes the key on the
host: 16/16-bit fields (wave, chain, chain_batch, kernel_search) or 20/20-bit ones (HBM).  Whatever the layout, the reported best
must be the minimum of the per-candidate (adds, muls) under the documented order -- cmpOpCount key of the cost mode, then seed:

  mode 0 (sum, then adds), mode 1 (adds, then muls), mode 2 (sum only).

In mode 2 the key holds only the sum.  The plan and chain searches ask the device again for the winner's split and report
(adds, muls); chain_batch and kernel_search report (sum, 0).
"""
import os

import pytest

from plo_testlib import DATA, OracleMatrix

pytestmark = pytest.mark.gpu
P = 131071
N = 64
SEED0 = 41
WRAP = 2**64 - 3                     # seed0 + offset passes 2^64 inside the launch


def _mat(name):
    M = OracleMatrix.from_sms(os.path.join(DATA, name), P)
    return (M.m, M.n, M.rowptr, M.col, M.val)


def _key(a, mu, mode):
    return (a, mu) if mode == 1 else (a + mu,) if mode == 2 else (a + mu, a)


def _expected(adds, muls, seed0, mode, split):
    """minimum under (key, offset); split: a sum-only key is reported as the winner's (adds, muls), otherwise as (sum, 0)"""
    k = min(range(len(adds)), key=lambda c: (_key(adds[c], muls[c], mode), c))
    a, mu = (adds[k], muls[k]) if mode != 2 or split else (adds[k] + muls[k], 0)
    return a, mu, (seed0 + k) % 2**64


def _plan(seed0, mode, hbm):
    from plinopt_amd import CSEPlan
    plan = CSEPlan(*_mat("cyclic.sms"), P, hbm=hbm)
    assert plan.is_hbm == hbm
    adds, muls = plan.cost_many(seed0=seed0, n=N)
    return plan.search(seed0, N, cost_mode=mode), _expected(adds, muls, seed0, mode, True)


def wave_plan(seed0, mode):
    return _plan(seed0, mode, False)


def hbm_plan(seed0, mode):
    return _plan(seed0, mode, True)


def chain(seed0, mode):
    from plinopt_amd import CSEChain
    ch = CSEChain(_mat("2x2x2_7_Winograd_L.sms"), _mat("cyclic.sms"), P)
    adds, muls = ch.cost_many(seed0=seed0, n=N)
    return ch.search(seed0, N, cost_mode=mode), _expected(adds, muls, seed0, mode, True)


def chain_batch(seed0, mode):
    from plinopt_amd import chain_batch
    pairs = [(_mat("2x2x2_7_Winograd_L.sms"), _mat("cyclic.sms")), (_mat("cyclic.sms"), _mat("2x2x2_7_Winograd_P.sms"))]
    adds, muls, best, _ = chain_batch(pairs, P, seed0, 8, cost_mode=mode)
    assert len(adds) == 16
    return best, _expected(adds, muls, seed0, mode, False)


def kernel_search(seed0, mode):
    from plinopt_amd import kernel_search
    adds, muls, _, best, _ = kernel_search(_mat("2x2x2_7_Winograd_L.sms"), P, seed0, N, cost_mode=mode)
    return best, _expected(adds, muls, seed0, mode, False)


ENTRIES = [wave_plan, hbm_plan, chain, chain_batch, kernel_search]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("entry", ENTRIES, ids=lambda f: f.__name__)
def test_best_is_the_minimum_of_the_entrys_own_costs(hip, entry, mode):
    got, exp = entry(SEED0, mode)
    assert got == exp


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda f: f.__name__)
def test_seed_offsets_that_wrap(hip, entry):
    got, exp = entry(WRAP, 0)
    assert got == exp
