"""The synthetic matrix of tests/test_gpu_sweep_pairs.py and tests/test_sweep_pairs_cases_host.py: the flat sweep of
plo::cse_big_kernel (mode 2, deferred updates) takes the entries of a row two at a time -- a lane's PAIR is entries 2j, 2j + 1 of one
row, loaded by one 8-byte load at a 4-byte aligned address -- so what matters is the parity of everything: of a row's length (the
odd slot of an odd row is inactive), of its start offset in the entry array, of the two removed positions pa < pb, and where a row
starts and ends relative to the 64 pairs of a trip.

  values    exactly 32 distinct residues mod 131071 (mode 2's limit), +-{1,2,3,4,5,6,9,10,12,15,18,20,25,30,45,50}: ratios are
            asymmetric (2/3 != 3/2), so a transposed ratio lookup of either entry of a pair changes a pair key, hence a frequency,
            hence the steps and the cost.
  groups    group g has f_g rows -- f_g / 2 shapes, each twice, so every triple has frequency >= 2 -- that hold columns a_g < b_g
            of its own (a_g = 100 + 100 g, b_g = a_g + 70, among 1000 columns) with v_b = r_g v_a.  The f_g are distinct
            and above every other frequency, and no row holds columns of two groups: the groups' prefix steps come first, in the
            order of f_g, and each finds its rows exactly as built.  A shape is (L, pa, pb): L entries, pa of them in columns left
            of a_g, pb - pa - 1 between a_g and b_g, the rest right of b_g, so the removed entries sit at positions pa and pb.

              g  f    value pairs (v_a, v_b), cycled                          shapes
              0  600  (2,3) (4,6) (6,9) (10,15)                               the 20 small shapes, then L = 2..9 at random
              1  96   (2,1) (4,2) (6,3) (10,5) (30,15) (-2,-1)                L = 65, 66: a long shape each; small; random
              2  80   (1,2) (2,4) (3,6) (5,10) (-1,-2) (15,30)                L = 127, 128
              3  72   (1,-1)                                                  L = 129, 130
              4  64   (1,1)                                                   small; random
              5  56   (-1,-1)
              6  48   (-1,1)
              7  40   (3,15) (2,10) (1,5) (6,30) (-3,-15)

            small shapes: every (pa, pb) of L = 2, 3, 4, 5 -- 20 of them: both length parities, the odd slot present and absent,
            a first, b last, pb = pa + 1 inside one pair (pa even) and across two (pa odd), and L = 2, where the new column's entry
            lands at position 0.  One long shape per length (LONG_SHAPES; more would cost the oracle seconds): together a first,
            b last in a row of odd and of even length, pb = pa + 1 inside one pair and across two, pa of either parity, and
            the three position classes in one row.  65, 66, 127, 128, 129, 130 entries are 33, 33, 64, 64, 65, 65 pairs: a
            lane's row changes inside a trip behind an odd and an even number of pairs, and a row ends exactly at, one pair
            before and one pair behind a trip's edge, shifted by the one to five pairs of each row before it in its wave.
            Group 0's step rewrites 600 rows: 75 per wave, a second batch of 11.
  filler    120 pairs of rows of 10 entries: triples enough, with the long rows', for the plan to take the deferred updates.
  order     the rows are shuffled, again until each of these ten lengths has a row at an even and a row at an odd start offset
            (the offset of a row in the entry array is the sum of the lengths before it).
"""
import random

P = 131071
MAGS = (1, 2, 3, 4, 5, 6, 9, 10, 12, 15, 18, 20, 25, 30, 45, 50)
VALS = sorted({x % P for x in MAGS} | {P - x for x in MAGS})
NCOLS = 1000
SMALL_LENGTHS = (2, 3, 4, 5)
LONG_LENGTHS = (65, 66, 127, 128, 129, 130)
GROUPS = (
    (600, ((2, 3), (4, 6), (6, 9), (10, 15)), ()),
    (96, ((2, 1), (4, 2), (6, 3), (10, 5), (30, 15), (-2, -1)), (65, 66)),
    (80, ((1, 2), (2, 4), (3, 6), (5, 10), (-1, -2), (15, 30)), (127, 128)),
    (72, ((1, -1),), (129, 130)),
    (64, ((1, 1),), ()),
    (56, ((-1, -1),), ()),
    (48, ((-1, 1),), ()),
    (40, ((3, 15), (2, 10), (1, 5), (6, 30), (-3, -15)), ()),
)
NFILLER = 120


def ab(g):
    return 100 + 100 * g, 170 + 100 * g


def small_shapes():
    return [(L, pa, pb) for L in SMALL_LENGTHS for pa in range(L) for pb in range(pa + 1, L)]


# one shape per long length (the literal oracle's time grows with the square of the long rows' entries): a first and pb = pa + 1 inside
# one pair; pa odd and pb = pa + 1 across two pairs; b last in a row of odd length; all three position classes; neighbours in the
# first pair of the row's second trip; b last in a row of even length
LONG_SHAPES = {65: (0, 1), 66: (1, 2), 127: (62, 126), 128: (43, 49), 129: (64, 65), 130: (64, 129)}


def shapes_of(g, rng):
    f, _, longs = GROUPS[g]
    out = [(L,) + LONG_SHAPES[L] for L in longs] + small_shapes()
    while len(out) < f // 2:
        L = rng.randrange(2, 10)
        pa = rng.randrange(0, L - 1)
        pb = rng.randrange(pa + 1, L)
        out.append((L, pa, pb))
    assert len(out) == f // 2
    return out


def matrix():
    """(rows as {column: value}, group of each row or -1, shape (L, pa, pb) of each group row or None)"""
    rng = random.Random(29)
    gcols = {c for g in range(len(GROUPS)) for c in ab(g)}
    others = [c for c in range(NCOLS) if c not in gcols]
    tagged = []
    for g, (f, pairs, _) in enumerate(GROUPS):
        a, b = ab(g)
        lo, mid, hi = [c for c in others if c < a], [c for c in others if a < c < b], [c for c in others if c > b]
        for k, (L, pa, pb) in enumerate(shapes_of(g, rng)):
            va, vb = pairs[k % len(pairs)]
            cols = rng.sample(lo, pa) + rng.sample(mid, pb - pa - 1) + rng.sample(hi, L - 1 - pb)
            row = {c: rng.choice(VALS) for c in cols}
            row[a], row[b] = va % P, vb % P
            srt = sorted(row)
            assert len(srt) == L and srt[pa] == a and srt[pb] == b
            tagged += [(dict(row), g, (L, pa, pb)), (dict(row), g, (L, pa, pb))]
    for _ in range(NFILLER):
        row = {c: rng.choice(VALS) for c in rng.sample(others, 10)}
        tagged += [(dict(row), -1, None), (dict(row), -1, None)]
    # shuffled until every length of interest starts at an even and at an odd offset (the offset of a row is the sum of the lengths before it)
    want = {(L, q) for L in SMALL_LENGTHS + LONG_LENGTHS for q in (0, 1)}
    while True:
        rng.shuffle(tagged)
        rs = row_starts([t[0] for t in tagged])
        if want <= {(t[2][0], o & 1) for t, o in zip(tagged, rs) if t[2]}:
            break
    return [t[0] for t in tagged], [t[1] for t in tagged], [t[2] for t in tagged]


def row_starts(rows):
    """offset of each row in the entry array: the CSR row pointer"""
    out, s = [], 0
    for r in rows:
        out.append(s)
        s += len(r)
    return out
