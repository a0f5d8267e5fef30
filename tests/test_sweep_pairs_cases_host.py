"""From the construction alone (no GPU): the matrix of tests/sweep_pairs_matrix.py holds every class of row, start offset and removed
position that tests/test_gpu_sweep_pairs.py claims to run through the flat sweep's pairs, its groups' steps come first and in order,
and the literal oracle finishes on it."""
import synth
from plo_testlib import OracleMatrix
from sweep_pairs_matrix import GROUPS, LONG_LENGTHS, NCOLS, P, SMALL_LENGTHS, VALS, ab, matrix, row_starts


def test_values_and_ratios():
    rows, _, _ = matrix()
    assert len(VALS) == 32 and {x for r in rows for x in r.values()} == set(VALS)          # exactly 32 distinct values: mode 2's limit
    inv = {x: pow(x, P - 2, P) for x in VALS}
    assert len({x * inv[y] % P for x in VALS for y in VALS}) < 1024
    assert any(x * inv[y] % P != y * inv[x] % P for x in VALS for y in VALS)               # asymmetric
    for g, (_, pairs, _) in enumerate(GROUPS):                                             # one ratio per group
        assert len({vb * pow(va, P - 2, P) % P for va, vb in pairs}) == 1
    assert any(pairs[0][0] * pow(pairs[0][1], P - 2, P) % P != pairs[0][1] * pow(pairs[0][0], P - 2, P) % P for _, pairs, _ in GROUPS)


def test_groups_come_first_and_in_order():
    """every group's triple (a_g, b_g, r_g) has frequency f_g; the f_g are distinct and every other triple lies below all of them (a
    triple with a created column is no more frequent than the triple of the same entry with a or b, which is counted here)"""
    rows, grp, _ = matrix()
    cnt = {}
    for r in rows:
        it = sorted(r.items())
        for i in range(len(it)):
            ci, vi = it[i]
            for j in range(i + 1, len(it)):
                k = (ci, it[j][0], vi * pow(it[j][1], -1, P) % P)
                cnt[k] = cnt.get(k, 0) + 1
    fs = [f for f, _, _ in GROUPS]
    assert len(set(fs)) == len(fs) and fs[0] == 600
    top = {}
    for g, f in enumerate(fs):
        a, b = ab(g)
        mine = [k for k in cnt if k[:2] == (a, b)]
        assert len(mine) == 1 and cnt[mine[0]] == f == grp.count(g)
        top[mine[0]] = f
        assert all((a in r) == (b in r) == (grp[i] == g) for i, r in enumerate(rows))     # nothing else holds its two columns
    assert max(c for k, c in cnt.items() if k not in top) < min(fs)


def test_row_and_position_classes():
    rows, grp, shp = matrix()
    rs = row_starts(rows)
    seen = set()
    for i, r in enumerate(rows):
        if grp[i] < 0:
            continue
        L, pa, pb = shp[i]
        a, b = ab(grp[i])
        cols = sorted(r)
        assert len(cols) == L and cols[pa] == a and cols[pb] == b
        big = L in LONG_LENGTHS
        seen |= {("len", L, "start", rs[i] & 1), ("pa", pa & 1, big), ("a first", pa == 0, big), ("b last", pb == L - 1, L & 1, big),
                 ("neighbours", pb == pa + 1, pa & 1, big), ("three classes", pa > 0 and pb > pa + 1 and pb < L - 1, big),
                 ("odd slot", L & 1), ("group 0", grp[i] == 0, L)}
    for L in SMALL_LENGTHS + LONG_LENGTHS:                    # every length at an even and at an odd start offset
        assert {("len", L, "start", 0), ("len", L, "start", 1)} <= seen, L
    for big in (False, True):                                 # short rows and rows that span trips
        assert {("pa", 0, big), ("pa", 1, big)} <= seen
        assert ("a first", True, big) in seen
        assert {("b last", True, 0, big), ("b last", True, 1, big)} <= seen                # b last in a row of even and of odd length
        assert {("neighbours", True, 0, big), ("neighbours", True, 1, big)} <= seen        # pb = pa + 1 inside one pair, across two
        assert ("three classes", True, big) in seen
    assert {("odd slot", 0), ("odd slot", 1)} <= seen
    assert ("group 0", True, 2) in seen                       # rows of two entries: the new column's entry lands at position 0
    # the long rows: a trip is 64 pairs
    assert sorted({(L + 1) // 2 for L in LONG_LENGTHS}) == [33, 64, 65]
    assert grp.count(0) == 600 and grp.count(0) > 512         # 75 rows per wave of 8: a second batch


def test_oracle_finishes():
    rows, _, _ = matrix()
    rp, c, v = synth.to_csr(rows, P)
    M = OracleMatrix(len(rows), NCOLS, rp, c, v, P)
    assert rp[:-1] == row_starts(rows)                        # the kernel keeps a row at its CSR offset
    adds, muls = M.cost_many(seed0=1, nseeds=1, nthreads=1)
    assert len(adds) == len(muls) == 1 and adds[0] > 0
