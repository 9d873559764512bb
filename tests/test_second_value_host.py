"""CPU tests of the second-value scan's definition: the big-integer reference of
tests/second_value_reference.py reproduces the classes and shifts stated by hand for the directed circuits, and on the random
circuits and the larger shape of tests/unbound_reference.py a two-valued wire's shift leaves every residual as it is, any other
change of it does not, and reading class 3 as BOUND gives the unbound-wire scan's classes."""
import functools

import pytest

import r1cs_builder as rb
import second_value_reference as sv
import unbound_reference as ur
import valid_key_builder as vkb
from second_value_reference import ABSENT, BOUND, R, ROOT, TWO_VALUED, UNBOUND


@pytest.mark.parametrize("name", sorted(sv.DIRECTED))
def test_reference_reproduces_the_hand_stated_classes_and_shifts(name):
    circ, classes, shifts = sv.DIRECTED[name]
    assert rb.check(*circ[1:]) == [], name                         # every directed witness satisfies its circuit
    assert sv.classify(*circ) == (classes, shifts), name
    assert all(0 < d < R for d in shifts.values())
    for wire, d in shifts.items():                                 # ... and the stated second value satisfies it too
        assert rb.check(*circ[1:4], sv.shifted(circ[4], wire, d)) == [], (name, wire)


def test_directed_set_holds_what_it_is_meant_to():
    d = sv.DIRECTED
    assert d["square_at_3"][2] == {1: R - 6} and d["square_at_0"][1] == [BOUND] * 3
    assert d["boolean_alone_0"][2] == {1: 1} and d["boolean_alone_1"][2] == {1: R - 1}
    assert d["quadratic_at_2"][2] == {1: 1} and d["quadratic_at_3"][2] == {1: R - 1}
    assert d["roots_agree"][1][1] == TWO_VALUED and d["roots_clash"][1][1] == BOUND
    kinds = sv.wire_kinds(*d["free_beside_root"][0])[1]
    assert sorted(k for _, k, _ in kinds) == [sv.FREE, ROOT]
    # coefficient products that equal those of x x = y0 only modulo r: as integers they pass r
    assert any(ka * kb > R and ka * kb % R == 1 for ka in ur.EXTREMES[1:] for kb in ur.EXTREMES[1:])
    assert len(d["extreme_factors"][0][1]) == 26
    for n, at, what in sv.COLUMN_CASES:
        circ, classes, _ = d["column_%d_%s_%s" % (n, what, at)]
        inc = ur.incidences(*circ[:4])
        assert [s for s, _, _, _, _ in inc if s] == [1] * n         # the walk is wire 1's column: incidence c = constraint c
        col = sv.wire_kinds(*circ)[1]
        odd = [c for c, k, dd in col if k != ROOT or dd != R - 2 * sv.X]
        assert odd == ([] if at is None else [at]), (n, at, what)
    for t in (255, 256, 257):
        for last in (sv.AGREE, sv.CLASH, sv.PINNED):
            circ, classes, _ = d["walked_%d_%s" % (t, last)]
            inc = ur.incidences(*circ[:4])
            assert sum(1 for s, _, _, _, _ in inc if s) == t        # walked: all but wire 0's column
            assert inc[-1][0] == circ[0] - 1                        # the last incidence is the highest wire's, and decides
            assert classes[-1] == (TWO_VALUED if last == sv.AGREE else BOUND) and classes.count(TWO_VALUED) >= t - 2
    for n in (64, 65, 128, 129):
        assert sorted(d["wires_%d" % n][2]) == [s for s in (63, 64, 127, 128) if s < n]


def columns(n_wires, rowsA, rowsB, rowsC):
    """per wire the constraints that name it in any term (unmerged): no other residual can move with it"""
    out = [set() for _ in range(n_wires)]
    for rows in (rowsA, rowsB, rowsC):
        for c, row in enumerate(rows):
            for s, _ in row:
                out[s].add(c)
    return [sorted(x) for x in out]


def assert_properties(circuit, w, what, whole):
    """whole: residuals of EVERY constraint (the small circuits); otherwise those of the wire's column, the only ones that name it"""
    n_wires, rowsA, rowsB, rowsC = circuit
    classes, shifts = sv.classify(n_wires, rowsA, rowsB, rowsC, w)
    cols = columns(*circuit)
    res = lambda ww, s: sv.residuals(rowsA, rowsB, rowsC, ww, None if whole else cols[s])
    for s, d in shifts.items():
        assert classes[s] == TWO_VALUED and 0 < d < R
        assert res(sv.shifted(w, s, d), s) == res(w, s), (what, s)
        for other in ((d + 1) % R, d - 1):                         # any change but 0 and d moves a residual (d = r - 1: d + 1 is 0)
            assert other == 0 or res(sv.shifted(w, s, other), s) != res(w, s), (what, s, other)
    for s, col in enumerate(sv.wire_kinds(n_wires, rowsA, rowsB, rowsC, w)):
        if s and classes[s] == BOUND:
            for _, k, d in col:
                if k == ROOT:
                    assert res(sv.shifted(w, s, d), s) != res(w, s), (what, s)
    assert [BOUND if k == TWO_VALUED else k for k in classes] == ur.classify(n_wires, rowsA, rowsB, rowsC, w), what
    return classes


def test_properties_on_the_random_circuits():
    two = 0
    for seed in range(ur.N_RANDOM):
        n_wires, rowsA, rowsB, rowsC, w, w_broken, _ = ur.random_circuit(seed)
        for ww in (w, w_broken):
            two += assert_properties((n_wires, rowsA, rowsB, rowsC), ww, seed, True).count(TWO_VALUED)
    assert two > 0


@functools.lru_cache(maxsize=None)
def large():
    shape = ur.large_shape()
    n_wires, rowsA, rowsB, rowsC, _ = rb.from_shape(shape)
    return (n_wires, rowsA, rowsB, rowsC), rb.witness_ints(vkb.fast_witness(shape, 5)[0])


def test_properties_on_the_larger_shape():
    circuit, w = large()
    classes = assert_properties(circuit, w, "large_shape", False)
    assert classes.count(TWO_VALUED) > 1000 and min(classes.count(k) for k in (BOUND, ABSENT, UNBOUND)) > 100
