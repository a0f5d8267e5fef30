"""tests/orbit_cse_cases.py against the oracles alone: the inputs of tests/test_gpu_orbiter_cse_edges.py are what their names say
(columns of the wide part, the lanes-per-row band it lands in, a row of exactly `columns` entries in the dense variants, more than
half of the 64-lane group active on the 64-lanes-per-row path, nothing above 64 in an accepted case and exactly one quantity
above 64 in a refused one), and the generator has not moved (sha256 of every case's text).  No GPU."""
import json
import os

import pytest

import orbit_cse_cases as cc
import synth
from plo_testlib import ROOT

PINS = json.load(open(os.path.join(ROOT, "tests", "golden", "orbit_cse_cases.json")))
PRIME = pytest.mark.parametrize("p", cc.PRIMES)


def short(c):
    return c.name.split("_", 2)[2]


@PRIME
def test_the_generator_has_not_moved(p):
    cases = cc.all_cases(p)
    assert len(cases) == 34 and len(PINS) == 34 * len(cc.PRIMES)
    for c in cases:
        assert c.sha256 == PINS[c.name] == synth._sha(synth.orbit_text(c)), c.name
        assert c.modulus == p and max(c.mkn) <= 16
    assert [short(c) for c in cases] == [short(c) for c in cc.all_cases(cc.PRIMES[0])]


@PRIME
def test_columns_and_bands(p):
    """the columns of hP are r, those of Lj mk, those of Rg kn; both sides of every lanes-per-row boundary occur"""
    hp = [c for c in cc.accepted(p) if short(c).startswith("hP_") and not c.dense]
    assert [(c.mkn, c.wide, c.cols, c.r) for c in hp] == [((2, 1, 2), cc.HP, r, r) for r in cc.HP_BANDS]
    assert [cc.band(c.cols) for c in hp] == [2, 3, 3, 4, 4, 5, 5, 6, 6, 6]
    for tag, part, bands in (("Lj_", cc.LJ, cc.LJ_BANDS), ("Rg_", cc.RG, cc.RG_BANDS)):
        got = [c for c in cc.accepted(p) if short(c).startswith(tag) and not c.dense]
        assert [(c.mkn, c.r) for c in got] == bands and all(c.wide == part for c in got)
        assert [c.cols for c in got] == [32, 33, 63, 64] == [cc.dims(c)[part][1] for c in got]
        assert [cc.band(c.cols) for c in got] == [5, 6, 6, 6]
    for c in cc.accepted(p):
        if c.wide is not None:
            assert c.cols == cc.dims(c)[c.wide][1] == max(cols for _, cols in cc.dims(c)), c.name
    # the row-count edges: 64 rows of hP; 64 rows of Lj and of Rg; one row of 64 columns
    assert cc.dims(cc.named(p, "rows_8x1x8_r3")) == [(3, 8), (3, 8), (64, 3)]
    assert cc.dims(cc.named(p, "hP_2x1x2_r64")) == [(64, 2), (64, 2), (4, 64)]
    assert cc.dims(cc.named(p, "rows_1x1x1_r64")) == [(64, 1), (64, 1), (1, 64)]


@PRIME
def test_dense_variants_have_a_full_row_under_the_base_seed(p):
    """every 33-, 63- and 64-column case has one; the image of the base candidate is the input, so the dense input row is a row of
    exactly `columns` entries of the image: a ballot with every bit of the row's lanes set, all 64 at 64 columns"""
    wide = cc.wide_cases(p)
    plain = [c for c in wide if not c.dense]
    assert sorted(c.cols for c in plain) == [33, 33, 33, 63, 63, 63, 64, 64, 64, 64]
    assert [short(c) for c in wide if c.dense] == [short(c) + "_dense" for c in plain]
    for c in wide:
        if c.dense:
            lens = cc.row_lengths(c, cc.BASE)[c.wide]
            assert max(lens) == c.cols and lens[0] == c.cols, c.name
    assert cc.row_lengths(cc.named(p, "rows_1x1x1_r64_dense"), cc.BASE)[cc.HP] == [64]                      # all of P


@PRIME
def test_more_than_half_of_the_wave_is_active_on_the_64_lane_path(p):
    """Over the listed seeds the wide part of every 33- to 64-column shape has a transformed row of more than 32 entries: with its
    dense variant for every shape, and on its own for the plain 64-column cases.  (A plain case of 33 columns would need a row
    without a zero, which sparse random rows do not give: 26 to 30 entries at p = 131071; the dense variant carries the shape.)"""
    longest = lambda c: max(max(cc.row_lengths(c, s)[c.wide]) for s in cc.SEEDS)  # noqa: E731
    for c in cc.wide_cases(p):
        top = longest(c)
        print(c.name, c.cols, top)
        assert top <= c.cols
        if c.dense or c.cols == 64:
            assert top > 32, c.name
        if c.dense and c.cols >= 63:
            # and not under the base seed alone: some drawn candidate keeps more than half of the lanes busy too
            assert max(max(cc.row_lengths(c, s)[c.wide]) for s in cc.SEEDS[1:]) > 32, c.name


@PRIME
def test_accepted_and_refused_sides_of_the_four_limits(p):
    for c in cc.accepted(p):
        assert max(cc.quantities(c).values()) <= 64 and c.refusal is None, c.name
        assert all(rows <= 64 and cols <= 64 for rows, cols in cc.dims(c)), c.name
    over = cc.refused(p)
    assert [c.quantity for c in over] == ["r", "mn", "mk", "kn"]
    for c in over:
        q = cc.quantities(c)
        assert [k for k, v in q.items() if v > 64] == [c.quantity] and q[c.quantity] == 65, c.name
        assert c.reason == ("r or mn above 64" if c.quantity in ("r", "mn") else "mk or kn above 64")
        assert synth.orbit_refusal(c) is None and c.waves >= 1, c.name          # the orbit plan's own limits accept it
    # the accepted sides: each quantity reaches 64
    tops = {k: max(cc.quantities(c)[k] for c in cc.accepted(p)) for k in ("r", "mn", "mk", "kn")}
    assert tops == {"r": 64, "mn": 64, "mk": 64, "kn": 64}


def test_images_are_tiny():
    """what the device has to hold: at most 246 entries in a part and 8192 table slots (64 KiB) by the sizing rule, on the seeds the
    GPU tests score"""
    ent = pairs = 0
    for p in cc.PRIMES:
        for c in cc.accepted(p):
            for s in cc.SEEDS:
                for lens in cc.row_lengths(c, s):
                    ent, pairs = max(ent, sum(lens)), max(pairs, cc.pair_instances(lens))
    print("largest part: %d entries, %d pair instances, %d slots" % (ent, pairs, cc.slots_for(pairs)))
    assert ent <= 256 and cc.slots_for(pairs) <= 8192


def test_sizing_rule():
    assert [cc.slots_for(x) for x in (0, 65, 66, 150, 151, 321, 322, 4800, 7448, 10902, 10903)] == [64, 64, 128, 128, 256, 256, 512, 4096, 8192, 8192, 16384]
    c = cc.named(131071, "rows_1x1x1_r64_dense")
    assert cc.table_slots(c) == (64, 64, cc.slots_for(64 * 63 // 2)) == (64, 64, 2048)
