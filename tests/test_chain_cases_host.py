"""The chained-candidate case family of tests/synth.py (chain_cases) against the CPU oracle alone: the family must be able to
tell a device that runs the random stream on from the first matrix to the second from one that restarts it, and one that
takes the pair in the given order from one that swaps it -- otherwise tests/test_gpu_chain_synth.py could pass on a wrong
kernel.  No GPU."""
import synth
from plo_testlib import OracleMatrix, oracle_chain

CASES = synth.chain_cases()
ADMITTED = [c for c in CASES if not c.refusal]


def mats(c):
    return [OracleMatrix(*(x.csr + (c.p,))) for x in (c.A, c.B)]


def all_seeds(c):
    return [c.run[0] + k for k in range(c.run[1])] + c.seeds


def independent(A, B, seeds):
    """Optimizer() on each matrix with a stream of its own per seed, costs added"""
    (aa, am), (ba, bm) = A.cost_many(seeds=seeds), B.cost_many(seeds=seeds)
    return [(w + y, x + z) for w, x, y, z in zip(aa, am, ba, bm)]


def test_family_shape():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert 45 <= len(CASES) <= 60
    assert {c.family for c in CASES} == {"order", "dispatch", "silent", "region", "mw", "rowlen", "moduli", "onewave", "refuse"}
    assert sorted(c.p for c in CASES if c.family == "moduli") == sorted(synth.CHAIN_MODULI * 2)
    for c in ADMITTED:
        if c.family == "onewave":
            assert len(set(all_seeds(c))) == 3                  # (the oracle's second per seed)
        else:
            assert c.run == synth.CHAIN_RUN and c.seeds == synth.CHAIN_SEEDS
        assert len(set(c.seeds)) < len(c.seeds)                 # a repeated seed in the explicit list


def test_matrices_are_valid_csr():
    for c in CASES:
        for x in (c.A, c.B):
            m, n, rp, col, val = x.csr
            assert (m, n) == (x.m, x.n) and len(rp) == m + 1 and rp[0] == 0 and rp[-1] == len(col) == len(val)
            for i in range(m):
                assert rp[i] <= rp[i + 1]
                row = col[rp[i]:rp[i + 1]]
                assert row == sorted(set(row)) and all(0 <= j < n for j in row)
            assert all(0 < v < c.p for v in val)


def test_oracle_scores_every_admitted_case():
    for c in ADMITTED:
        A, B = mats(c)
        for s in all_seeds(c):
            a, mu = oracle_chain(A, B, s)
            assert 0 <= a < 1 << 16 and 0 <= mu < 1 << 16, (c.name, s)


def test_order_cases_tell_a_continuing_stream_from_a_restarted_one():
    seeds = list(range(64))
    differ = {}
    for c in CASES:
        if c.family == "order":
            A, B = mats(c)
            chained = [oracle_chain(A, B, s) for s in seeds]
            differ[c.name] = sum(x != y for x, y in zip(chained, independent(A, B, seeds)))
    assert max(differ.values()) >= 8, differ


def test_order_cases_tell_the_order_of_the_pair():
    swapped = {}
    for c in CASES:
        if c.family == "order":
            A, B = mats(c)
            swapped[c.name] = sum(oracle_chain(A, B, s) != oracle_chain(B, A, s) for s in range(64))
    assert max(swapped.values()) >= 1, swapped


def test_a_silent_first_matrix_leaves_the_stream_untouched():
    seen = 0
    for c in CASES:
        if c.family == "silent" and c.silent_first:
            A, B = mats(c)
            seeds = all_seeds(c)
            assert [oracle_chain(A, B, s) for s in seeds] == independent(A, B, seeds), c.name
            seen += 1
    assert seen == 3                                            # all rows empty, 1 x 1, no pair of frequency 2
