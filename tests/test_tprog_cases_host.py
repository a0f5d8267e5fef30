"""The cases of tests/tprog_cases.py themselves, under their own definition: every generated program is correct, every mutation is
violated in the blocks it aims at, the definition agrees with the interpreter of plo_testlib on random inputs, and the
certificate rule in exact integers bounds the cleared defects.  No GPU, no tool."""
import random
from fractions import Fraction

import pytest

import tprog_cases as C
from plo_testlib import LowHigh, run_inplace_program

EDGE = C.edge_cases("issue") + C.edge_cases("units")
MUT = C.mutations() + C.mutations(C.schoolbook(3, 5, True, "units"))


def block_of(case, e):
    if e < case.E0:
        return 0
    e -= case.E0
    return 1 if e < case.na ** 2 else 2 if e < case.na ** 2 + case.nb ** 2 else 3


@pytest.mark.parametrize("case", EDGE, ids=lambda c: c.name)
def test_generated_programs_are_correct(case):
    assert C.definition(case) == (0, None, None, None)
    for q in (131071, C.P31, C.P62):
        assert C.definition(case, q) == (0, None, None, None)
    for q in (3, 15):
        if "units" in case.name:
            assert C.definition(case, q) == (0, None, None, None)
        else:
            with pytest.raises(C.Refused) as r:
                C.definition(case, q)
            assert r.value.kind == "unit" and r.value.line is not None


def test_programs_hold_every_kind_of_line():
    for case in (C.schoolbook(2, 65), C.schoolbook(2, 65, True)):
        for pat in (r"a\d+:=a\d+\*3;", r"c\d+:=c\d+/3;", r"b\d+:=b\d+\*-5/3;", r"b\d+:=-b\d+/2;", r"c\d+:=-c\d+\*2;", r"c\d+:=c\d+\+c\d+/2;", r"a\d+:=a\d+\+a\d+\*3;", r"b\d+:=b\d+-b\d+/2;"):
            assert C.re.search("(?m)^" + pat, case.text), pat
    recs = C.parse(C.schoolbook(2, 65).text, 2, 65, 66, False)
    assert sum(r[1] == C.AXPY for r in recs) > 2 * 65                          # the compensating AXPYs: some alpha are not unit vectors


@pytest.mark.parametrize("case", [C.schoolbook(2, 5), C.schoolbook(3, 4, True), C.schoolbook(1, 5), C.mutations()[1][0], C.mutations()[8][0]], ids=lambda c: c.name)
def test_definition_agrees_with_the_interpreter_on_random_inputs(case):
    """c' = C c + S(a, b), a' = A a, b' = B b: the final state that the definition's defects predict is what
    run_inplace_program computes"""
    rnd = random.Random(len(case.text))
    bad = C.defects(case)
    a0 = [Fraction(rnd.randint(-9, 9), rnd.randint(1, 5)) for _ in range(case.na)]
    b0 = [Fraction(rnd.randint(-9, 9), rnd.randint(1, 5)) for _ in range(case.nb)]
    c0 = [Fraction(rnd.randint(-9, 9), rnd.randint(1, 5)) for _ in range(case.nc)]
    a, b, c = list(a0), list(b0), [LowHigh(x) for x in c0] if case.expanded else list(c0)
    run_inplace_program(case.text, a, b, c)
    T = C.target(case)
    S = {}
    for (i, j, z), v in T.items():
        for e in ([(i * case.nb + j) * case.w + z, (i * case.nb + j) * case.w + case.nc + z + 1] if case.expanded else [(i * case.nb + j) * case.w + z]):
            S[e] = v
    for e, (got, _) in bad.items():
        if e < case.E0:
            S[e] = got
    lin = []
    e0 = case.E0
    for n in (case.na, case.nb, case.nc):
        lin.append([[bad.get(e0 + x * n + i, (Fraction(int(x == i)),))[0] for i in range(n)] for x in range(n)])
        e0 += n * n
    assert a == [sum(lin[0][x][i] * a0[i] for i in range(case.na)) for x in range(case.na)]
    assert b == [sum(lin[1][x][i] * b0[i] for i in range(case.nb)) for x in range(case.nb)]
    for z in range(case.nc):
        plain = sum(lin[2][z][i] * c0[i] for i in range(case.nc))
        bil = [sum(S.get((i * case.nb + j) * case.w + h + z, 0) * a0[i] * b0[j] for i in range(case.na) for j in range(case.nb)) for h in range(0, case.w, case.nc)]
        assert c[z] == (LowHigh(plain, bil[0], bil[1]) if case.expanded else plain + bil[0]), z


@pytest.mark.parametrize("mut", MUT, ids=lambda m: m[0].name)
def test_mutations_are_violated_where_they_aim(mut):
    case, blocks = mut
    bad = C.defects(case)
    assert bad and {block_of(case, e) for e in bad} >= blocks
    violated, first, found, expected = C.definition(case)
    assert violated == len(bad) and first == min(bad) and found != expected
    assert block_of(case, first) == min(blocks)                                # bilinear first when both kinds are violated
    if blocks == {0, 3}:
        assert {block_of(case, e) for e in bad} == {0, 3}
    assert C.definition(case, 131071)[0] >= 1


def test_hidden_defect_is_a_multiple_of_the_first_prime():
    case = C.hidden_defect()
    violated, first, found, expected = C.definition(case)
    assert (violated, found, expected) == (1, C.P31, 0) and block_of(case, first) == 3
    assert C.definition(case, C.P31) == (0, None, None, None)
    assert C.definition(case, 2147483587)[0] == 1
    assert C.certificate(case)[1] >= 2


@pytest.mark.parametrize("case", [m for m, _ in MUT] + [C.hidden_defect()], ids=lambda c: c.name)
def test_certificate_bounds_the_cleared_defects(case):
    beta, j = C.certificate(case)
    assert beta >= C.cleared_defect_bits(case) and j == -(-beta // 30)


def test_pair_ranges_of_the_definition():
    case = C.mutations()[0][0]
    violated, first, _, _ = C.definition(case)
    pair = first // case.w
    assert C.definition(case, 0, pair, pair + 1)[:2] == (violated, first)
    assert C.definition(case, 0, 0, pair) == (0, None, None, None)
    ra = C.mutations()[5][0]                                                   # a restoration block goes with ranges from pair 0 only
    assert C.definition(ra, 0, 0, 1)[0] == 1 and C.definition(ra, 0, 1, 2)[0] == 0


@pytest.mark.parametrize("line,kind", C.REFUSED)
def test_the_definition_refuses(line, kind):
    with pytest.raises(C.Refused) as r:
        C.parse("# head\na0:=a0*3;\n" + line + "\n", 2, 3, 4, False)
    assert (r.value.line, r.value.kind) == (3, kind)


def test_the_definition_ignores_what_the_grammar_ignores():
    text = "# a0:=junk;\n\nplain words\na0:=a0*3; ### anything := here ###\n  a0 := a0 / 3 ;\n"
    assert [r[1] for r in C.parse(text, 1, 1, 1, False)] == [C.SCA, C.SCA]
    with pytest.raises(C.Refused) as r:
        C.parse("c0:=c0 + a0 * b0;\n", 1, 1, 2, True)
    assert r.value.kind == "plain"
