"""Big-integer reference of the second-value scan (include/k16.h k16_r1cs_second_values) and the
circuits its tests share.  Straight from the definition, in Python integers; it shares no code with the product.

For wire i and constraint c, with the merged coefficients A^, B^, C^ and the sums a = A_c.w, b = B_c.w,
    lin = A^ b + B^ a - C^,   quad = A^ B^   (mod r)
and changing wire i alone by d moves the residual a b - c of constraint c by d lin + d^2 quad.  An incidence is FREE (both zero),
a PIN (exactly one zero) or a ROOT (neither zero, d = -lin / quad).  A wire is TWO_VALUED when it has no PIN, at least one ROOT
and all its ROOTs give the same d, its shift; every other wire keeps its class of the unbound-wire scan."""
import functools

import pymodel as pm
import r1cs_builder as rb
import unbound_reference as ur
from unbound_reference import ABSENT, BOUND, EXTREMES, UNBOUND

R = pm.R
TWO_VALUED = 3
FREE, PIN, ROOT = "free", "pin", "root"


@functools.lru_cache(maxsize=4096)
def inverse(x):
    return pow(x, R - 2, R)


def kind(ka, kb, kc, a, b):
    """(FREE | PIN | ROOT, d or None) of one incidence"""
    lin, quad = (ka * b + kb * a - kc) % R, ka * kb % R
    if lin == 0 and quad == 0:
        return FREE, None
    if lin == 0 or quad == 0:
        return PIN, None
    return ROOT, -lin * inverse(quad) % R


def wire_kinds(n_wires, rowsA, rowsB, rowsC, w):
    """per wire: [(constraint, kind, d)] over its incidences, ascending by constraint"""
    a = [rb.dot(r, w) for r in rowsA]
    b = [rb.dot(r, w) for r in rowsB]
    out = [[] for _ in range(n_wires)]
    for s, c, ka, kb, kc in ur.incidences(n_wires, rowsA, rowsB, rowsC):
        out[s].append((c,) + kind(ka, kb, kc, a[c], b[c]))
    return out


def classify(n_wires, rowsA, rowsB, rowsC, w):
    """(classes 0 .. 3 of every wire, {two-valued wire: shift})"""
    classes, shifts = [BOUND], {}
    for s, col in enumerate(wire_kinds(n_wires, rowsA, rowsB, rowsC, w)):
        if s == 0:
            continue
        ds = {d for _, k, d in col if k == ROOT}
        if not col:
            classes.append(ABSENT)
        elif all(k == FREE for _, k, _ in col):
            classes.append(UNBOUND)
        elif len(ds) == 1 and not any(k == PIN for _, k, _ in col):
            classes.append(TWO_VALUED)
            shifts[s] = ds.pop()
        else:
            classes.append(BOUND)
    return classes, shifts


def summary(classes, shifts):
    """(n, ascending two-valued wires, their shifts) as k16_r1cs_second_values reports them"""
    two = [s for s, k in enumerate(classes) if k == TWO_VALUED]
    return len(two), two, [shifts[s] for s in two]


def residuals(rowsA, rowsB, rowsC, w, constraints=None):
    cs = range(len(rowsA)) if constraints is None else constraints
    return [(rb.dot(rowsA[c], w) * rb.dot(rowsB[c], w) - rb.dot(rowsC[c], w)) % R for c in cs]


def shifted(w, wire, d):
    w2 = list(w)
    w2[wire] = (w2[wire] + d) % R
    return w2


# ---------------------------------------------------------------- directed circuits
# name -> ((n_wires, rowsA, rowsB, rowsC, w), classes of every wire, {two-valued wire: shift}); classes and shifts are stated
# by hand here and compared with classify() in tests/test_second_value_host.py.
ONE = [(0, 1)]
X = 3                                                              # the value of the wire under test where none is named


def const(k):
    return [(0, k % R)]


def square(x):
    """x x = y, y one = x^2 over wires 1 x, 2 y: lin = 2 x, quad = 1 for x; y has C^ = 1 in the first row, a PIN"""
    circ = 3, [[(1, 1)], [(2, 1)]], [[(1, 1)], ONE], [[(2, 1)], const(x * x)], [1, x, x * x % R]
    return (circ, [BOUND, TWO_VALUED, BOUND], {1: -2 * x % R}) if x else (circ, [BOUND, BOUND, BOUND], {})


def boolean(b, used):
    """b (b - one) = 0; used: also b one = out.  lin = (b - 1) + b, quad = 1: d = 1 at b = 0, -1 at b = 1"""
    rowsA, rowsB, rowsC = [[(1, 1)]], [[(1, 1), (0, R - 1)]], [[]]
    if not used:
        return (2, rowsA, rowsB, rowsC, [1, b]), [BOUND, TWO_VALUED], {1: 1 if b == 0 else R - 1}
    return (3, rowsA + [[(1, 1)]], rowsB + [ONE], rowsC + [[(2, 1)]], [1, b, b]), [BOUND, BOUND, BOUND], {}


def two_squares(clash):
    """x x = y1 beside (2x)(3x) = y2 (lin = 12 x, quad = 6: the same d = -2x) or beside x (x - one) = y2 (d = -(2x - 1))"""
    x = X
    if clash:
        rowsA, rowsB, y2 = [[(1, 1)], [(1, 1)]], [[(1, 1)], [(1, 1), (0, R - 1)]], x * (x - 1)
    else:
        rowsA, rowsB, y2 = [[(1, 1)], [(1, 2)]], [[(1, 1)], [(1, 3)]], 6 * x * x
    circ = 4, rowsA, rowsB, [[(2, 1)], [(3, 1)]], [1, x, x * x, y2]
    return (circ, [BOUND, BOUND, BOUND, BOUND], {}) if clash else (circ, [BOUND, TWO_VALUED, BOUND, BOUND], {1: R - 2 * x})


def quadratic(x):
    """x x = 5 x - 6 (roots 2 and 3): C^ = 5 is in lin = 2 x - 5, quad = 1"""
    return (2, [[(1, 1)]], [[(1, 1)]], [[(1, 5), (0, R - 6)]], [1, x]), [BOUND, TWO_VALUED], {1: (5 - 2 * x) % R}


def listed_twice():
    """(x + x) x = y: A^ = 2 is a sum (the side table); lin = 2 x + 2 x, quad = 2: d = -2 x"""
    x = X
    return (3, [[(1, 1), (1, 1)]], [[(1, 1)]], [[(2, 1)]], [1, x, 2 * x * x]), [BOUND, TWO_VALUED, BOUND], {1: R - 2 * x}


def extreme_factors():
    """x x = y0 and (ka x)(kb x) = ka kb x^2 for every pair of EXTREMES[1:]: lin = 2 ka kb x, quad = ka kb, d = -2 x in all
    of them, yet the cross-products lin quad0 and lin0 quad are equal only modulo r ((r - 1)^2 against 1)"""
    x = X
    rowsA, rowsB, rowsC = [[(1, 1)]], [[(1, 1)]], [const(x * x)]
    for ka in EXTREMES[1:]:
        for kb in EXTREMES[1:]:
            rowsA.append([(1, ka)]), rowsB.append([(1, kb)]), rowsC.append(const(ka * kb * x * x))
    return (2, rowsA, rowsB, rowsC, [1, x]), [BOUND, TWO_VALUED], {1: R - 2 * x}


def negated_square():
    """(-x)(-x) = y alone: quad = (r - 1)^2 = 1 modulo r"""
    x = X
    return (3, [[(1, R - 1)]], [[(1, R - 1)]], [[(2, 1)]], [1, x, x * x]), [BOUND, TWO_VALUED, BOUND], {1: R - 2 * x}


def free_beside_root():
    """x (k one) = k x, a FREE row, beside x x = x^2"""
    x, k = X, R - 2
    return (2, [[(1, 1)], [(1, 1)]], [const(k), [(1, 1)]], [[(1, k)], const(x * x)], [1, x]), [BOUND, TWO_VALUED], {1: R - 2 * x}


AGREE, CLASH, PINNED = "agree", "clash", "pin"


def column_row(c, what, x):
    """one row on wire 1 (C on wire 0, which is no variable): (k x) x = k x^2 with d = -2 x; a clash x (x - one) = x^2 - x
    with d = -(2 x - 1); a PIN x one = x"""
    if what == CLASH:
        return [(1, 1)], [(1, 1), (0, R - 1)], const(x * x - x)
    if what == PINNED:
        return [(1, 1)], ONE, const(x)
    k = EXTREMES[1 + c % 5]
    return [(1, k)], [(1, 1)], const(k * x * x)


COLUMN_CASES = [(n, at, what) for n in (1, 63, 64, 65, 129, 257) for what in (CLASH, PINNED)
                for at in sorted({0, 63, 64, n - 1} & set(range(n))) + [None]]


def column(n, at, what):
    """wire 1 in n agreeing ROOT constraints, constraint `at` (None: none) made a clash or a PIN.  Wire 1's column is all the scan
    walks: incidence c is constraint c, so `at` is the deciding LANE, and at = 0 makes the odd one the reference"""
    x = X
    rows = [column_row(c, what if c == at else AGREE, x) for c in range(n)]
    circ = 2, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [1, x]
    if at is None or (n == 1 and what == CLASH):                   # (a lone clash row is a lone ROOT)
        return circ, [BOUND, TWO_VALUED], {1: (1 - 2 * x) % R if at is not None else R - 2 * x}
    return circ, [BOUND, BOUND], {}


def walked(target, last):
    """exactly `target` walked incidences, none on a wire other than its own: the wires 1 .. target - 2 in one square each,
    s s = w_s^2 (two-valued), the LAST wire in two rows: a square and the deciding last incidence, agreeing, clashing or a PIN"""
    n_wires = target
    w = [1] + [2 + s % 5 for s in range(1, n_wires)]
    rowsA = [[(s, 1)] for s in range(1, n_wires)]
    rowsB = [[(s, 1)] for s in range(1, n_wires)]
    rowsC = [const(w[s] * w[s]) for s in range(1, n_wires)]
    s, x = n_wires - 1, w[n_wires - 1]
    a, b, c = column_row(1, last, x)
    rowsA.append([(s, k) for _, k in a]), rowsB.append([(s if t else 0, k) for t, k in b]), rowsC.append(c)
    classes = [BOUND] + [TWO_VALUED] * (n_wires - 2) + [TWO_VALUED if last == AGREE else BOUND]
    shifts = {t: R - 2 * w[t] for t in range(1, n_wires) if classes[t] == TWO_VALUED}
    return (n_wires, rowsA, rowsB, rowsC, w), classes, shifts


def word_edges(n_wires):
    """every wire single (s one = w_s) except 63, 64, 127 and 128, which sit in a square alone"""
    two = {s for s in (63, 64, 127, 128) if s < n_wires}
    w = [1] + [2 + s % 7 for s in range(1, n_wires)]
    rowsA = [[(s, 1)] for s in range(1, n_wires)]
    rowsB = [[(s, 1)] if s in two else ONE for s in range(1, n_wires)]
    rowsC = [const(w[s] * w[s] if s in two else w[s]) for s in range(1, n_wires)]
    classes = [BOUND] + [TWO_VALUED if s in two else BOUND for s in range(1, n_wires)]
    return (n_wires, rowsA, rowsB, rowsC, w), classes, {s: R - 2 * w[s] for s in two}


DIRECTED = {
    "square_at_3": square(3), "square_at_0": square(0),
    "boolean_alone_0": boolean(0, False), "boolean_alone_1": boolean(1, False),
    "boolean_used_0": boolean(0, True), "boolean_used_1": boolean(1, True),
    "roots_agree": two_squares(False), "roots_clash": two_squares(True),
    "quadratic_at_2": quadratic(2), "quadratic_at_3": quadratic(3),
    "listed_twice": listed_twice(), "extreme_factors": extreme_factors(), "negated_square": negated_square(),
    "free_beside_root": free_beside_root(),
}
DIRECTED.update({"column_%d_%s_%s" % (n, what, at): column(n, at, what) for n, at, what in COLUMN_CASES})
DIRECTED.update({"walked_%d_%s" % (t, last): walked(t, last) for t in (255, 256, 257) for last in (AGREE, CLASH, PINNED)})
DIRECTED.update({"wires_%d" % n: word_edges(n) for n in (64, 65, 128, 129)})
