"""Writes tests/golden/dependency_hits.json from the literal oracle tests/dependency_oracle.py: per case the coefficient line,
the numbers of vanishing and of canonical combinations, and the stdout text of `dependency` (in full up to 400 lines,
otherwise its line count and sha256).  Fixture cases name a file of tests/golden/data; synthetic ones carry their matrix
as SMS text.  Run once (the largest case takes tens of seconds): python tests/golden/make_dependency_hits.py"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dependency_oracle as D  # noqa: E402

FULL_TEXT_LINES = 400
P31 = 2147483629

# (fixture, -l, -c, -q, -v)
FIXTURES = [
    ("2x2x2_7_Winograd_L", 4, 11, 0, ""),
    ("2x2x2_7_Winograd_P", 4, 11, 0, ""),
    ("2x2x2_7_DPS-accurate_L", 3, 11, 0, ""),
    ("3x3x3_23_58_L", 3, 3, 0, ""),
    ("4x4x4_48_rational_L", 2, 11, 0, ""),
    ("3x4x7_63_rational_R", 2, 7, 0, ""),
    ("4x4x4_49_156_L", 3, 5, 0, ""),
    ("2x2x2_7_Winograd_L", 4, 11, 7, ""),
    ("2x2x2_7_Strassen_L", 4, 11, 3, ""),
    # the coefficient line and the levels
    ("2x2x2_7_Winograd_L", 2, 11, 0, "3 1/2"),
    ("2x2x2_7_Winograd_L", 3, 1, 0, ""),
    ("2x2x2_7_Winograd_L", 1, 11, 0, ""),
    ("2x2x2_7_Winograd_L", 0, 2, 0, ""),
]
# the prototype's counts of the issue: (zero, canonical) per fixture case above
EXPECTED = {0: (6, 233), 1: (0, 0), 2: (3, 25), 3: (13, 100), 4: (0, 16), 5: (0, 45), 6: (42, 208), 7: (6, 151), 8: (6, 46)}


def lcg(seed):
    s = seed
    while True:
        s = (s * 1103515245 + 12345) % (1 << 31)
        yield s >> 8


def dense_rows(mat):
    return [[(j, D.Fraction(x)) for j, x in enumerate(r) if x != 0] for r in mat]


def rnd_matrix(m, n, seed, vals=(-1, 0, 0, 1, 1, 2)):
    g = lcg(seed)
    return [[vals[next(g) % len(vals)] for _ in range(n)] for _ in range(m)]


def wide(n, seed):
    """5 rows of n columns: row 1 = row 0 but for one column, row 3 = row 0 + row 2, row 4 = 2 row 2 (hits that need every column)"""
    a, b = rnd_matrix(2, n, seed, vals=(1, 2, 3, -1, -2))
    r1 = list(a); r1[n - 1] += 1
    return [a, r1, b, [x + y for x, y in zip(a, b)], [2 * y for y in b]]


def synthetic():
    a, b, c = [1, 2, 0, 0, 1, 0], [0, 1, 1, 0, 0, 3], [0, 0, 2, 1, 1, 0]
    s234 = [[x + y + z for x, y, z in zip(a, b, c)], a, b, c, [x + y for x, y in zip(a, b)], a]
    # (name, matrix, -l, -c, -q)
    return [
        ("m1", [[1, 2, 3]], 4, 11, 0),
        ("m2_level_above_m", [[1, 2, 0], [1, 2, 1]], 4, 11, 0),
        ("n1_m12", [[1]] * 12, 3, 3, 0),
        ("n64", wide(64, 5), 3, 4, 0),
        ("n65", wide(65, 6), 3, 4, 0),
        ("n65_mod", wide(65, 6), 3, 4, 131071),
        ("last63", rnd_matrix(11, 3, 7), 3, 7, 0),
        ("last64", rnd_matrix(10, 3, 8), 3, 8, 0),
        ("last65", rnd_matrix(15, 3, 9), 3, 5, 0),
        ("level2", rnd_matrix(9, 3, 10), 2, 6, 0),
        ("sizes234", s234, 4, 3, 0),
        ("zero_and_duplicate_rows", [[1, 2, 3], [0, 0, 0], [2, 0, 1], [1, 2, 3]], 3, 4, 0),
        ("zero_and_duplicate_rows", [[1, 2, 3], [0, 0, 0], [2, 0, 1], [1, 2, 3]], 3, 4, 5),
        ("filter_false_hit", [[1, P31 + 1, 2 * P31 + 1], [1, 1, 1]], 2, 2, 0),
        ("filter_zero_is_canonical", [[1, P31 + 1], [1, 1]], 2, 2, 0),
    ]


def record(m, n, rows, lvl, c, q, v):
    head, hits = D.depender(m, n, rows, level=lvl, maxnum=c, extra=v.split(), q=q)
    text = D.text_of(hits)
    rec = {"l": lvl, "c": c, "q": q, "v": v, "head": head, "zero": sum(1 for h in hits if h[2] == 0), "canonical": sum(1 for h in hits if h[2] == 1),
           "sizes": sorted(set(len(h[0]) for h in hits)), "lines": len(hits), "sha256": hashlib.sha256(text.encode()).hexdigest()}
    if len(hits) <= FULL_TEXT_LINES:
        rec["text"] = text
    return rec


def main():
    out = {"fixtures": [], "synthetic": []}
    for k, (name, lvl, c, q, v) in enumerate(FIXTURES):
        m, n, rows = D.load_sms(os.path.join(HERE, "data", name + ".sms"))
        rec = record(m, n, rows, lvl, c, q, v)
        rec["input"] = name
        if k in EXPECTED:
            assert (rec["zero"], rec["canonical"]) == EXPECTED[k], (name, rec["zero"], rec["canonical"])
        out["fixtures"].append(rec)
        print(name, lvl, c, q, repr(v), rec["zero"], rec["canonical"], file=sys.stderr)
    for name, mat, lvl, c, q in synthetic():
        rows = dense_rows(mat)
        rec = record(len(mat), len(mat[0]), rows, lvl, c, q, "")
        rec["input"] = name
        rec["sms"] = D.to_sms(len(mat), len(mat[0]), rows)
        out["synthetic"].append(rec)
        print(name, lvl, c, q, rec["zero"], rec["canonical"], rec["sizes"], file=sys.stderr)
    by = {r["input"]: r for r in out["synthetic"]}
    assert by["n1_m12"]["lines"] == 2178
    assert by["sizes234"]["sizes"] == [2, 3, 4]
    assert by["filter_false_hit"]["lines"] == 0 and "i1*2147483629" in by["filter_zero_is_canonical"]["text"]
    with open(os.path.join(HERE, "dependency_hits.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
