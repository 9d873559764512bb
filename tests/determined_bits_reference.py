"""Big-integer reference of the determinism closure's bit rule (include/k16.h k16_r1cs_determined_wires_ex and
k16_r1cs_held_wires), an independent replayer of its certificates, and the circuits its tests share.
Straight from the definition, in Python integers, on top of determined_reference (the PIN rule's levels, run from the current
set of known wires) and solve_bits_reference (the marking rows, the gadgets); it edits neither.

A case is (circuit, w, header, seed) as in determined_reference; `seed` is always a list here.

HELD: wire x >= 1, some constraint that marks x BOOLEAN (solve_bits_reference.boolean_form) is not broken by w.
THE BIT RULE with respect to K: constraint c not broken by w, outside wires x_1 < .. < x_k (merged coefficient non-zero, not in
K), 2 <= k <= 253; (a) all HELD; (b) A^ = 0 on every outside wire or B^ = 0 on every outside wire; lin_j = A^_j b + B^_j a - C^_j
with a, b the sums of c under w (by (b) the one that multiplies an unknown is a sum over K); (c) lambda = lin of x_1, else of x_k
(0 is no lambda): every lin_j / lambda is 2^(e_j) as a canonical integer, e_j distinct, <= 252.  Then every x_j joins K.
LEVELS: the PIN rule's fixed point, ONE bit level (round = the next number, by = the lowest qualifying c naming x, rule 2), the
PIN rule again, until a bit level derives nothing."""
import functools
import itertools

import determined_reference as dr
import pymodel as pm
import r1cs_builder as rb
import solve_bits_reference as sb
import unbound_reference as ur
from determined_reference import ABSENT, DERIVED, NONE, OPEN, SEED, const, v
from solve_bits_reference import Circuit, below

R = pm.R
PIN, BITS = 1, 2
MAX_EXP = 252
inv = lambda t: pow(t, R - 2, R)


def marking_rows(circuit):
    """[(constraint, the wire it marks BOOLEAN)], ascending"""
    return [(c, x) for c, x in ((c, sb.boolean_form(*ms)) for c, ms in enumerate(sb.merged_of(circuit))) if x is not None]


def held_wires(circuit, w):
    """[0 / 1 per wire]"""
    _, rowsA, rowsB, rowsC = circuit
    broken = set(rb.check(rowsA, rowsB, rowsC, w))
    mark = [0] * circuit[0]
    for c, x in marking_rows(circuit):
        if c not in broken:
            mark[x] = 1
    return mark


def exponents(lins):
    """(c) on the lins of the outside wires in ascending wire order: the exponents, or None"""
    for lam in (lins[0], lins[-1]):
        if lam == 0:
            continue
        back = inv(lam)
        ratios = [l * back % R for l in lins]
        if any(t == 0 or t & (t - 1) or t.bit_length() - 1 > MAX_EXP for t in ratios):
            continue
        exps = [t.bit_length() - 1 for t in ratios]
        if len(set(exps)) == len(exps):
            return exps
    return None


def bit_row(ms, a, b, known, held):
    """one unbroken constraint with merged rows ms and sums a, b with respect to the known set: the outside wires it gives, or
    None"""
    ma, mb, mc = ms
    out = sorted(s for s in set(ma) | set(mb) | set(mc) if s not in known)
    if not 2 <= len(out) <= MAX_EXP + 1:
        return None
    if not all(held[x] for x in out):
        return None                                                                  # (a)
    if any(x in ma for x in out) and any(x in mb for x in out):
        return None                                                                  # (b)
    lins = [(ma.get(x, 0) * b + mb.get(x, 0) * a - mc.get(x, 0)) % R for x in out]
    return out if exponents(lins) is not None else None                              # (c)


def closure(circuit, w, seed, rules=PIN | BITS):
    """dict: status, round, by, rule (0 / 1 / 2) of every wire, n_by_bits"""
    assert rules in (PIN, PIN | BITS)
    n_wires, rowsA, rowsB, rowsC = circuit
    merged = sb.merged_of(circuit)
    held = held_wires(circuit, w)
    broken = set(rb.check(rowsA, rowsB, rowsC, w))
    sums = [(rb.dot(ra, w), rb.dot(rb_, w)) for ra, rb_ in zip(rowsA, rowsB)]
    in_seed = set(seed) | {0}
    known = set(in_seed)
    rounds, by, rule = {s: 0 for s in in_seed}, {}, {}
    level = 0
    while True:
        status, ro, b = dr.closure(circuit, w, sorted(known))                         # the PIN rule from K
        depth = 0
        for s in range(n_wires):
            if status[s] == DERIVED:
                known.add(s)
                rounds[s], by[s], rule[s] = level + ro[s], b[s], PIN
                depth = max(depth, ro[s])
        level += depth
        if not rules & BITS:
            break
        new = {}
        for c, ms in enumerate(merged):                                               # ascending: the first claim is the lowest
            if c in broken:
                continue
            for x in bit_row(ms, sums[c][0], sums[c][1], known, held) or ():
                new.setdefault(x, c)
        if not new:
            break
        level += 1
        for x, c in new.items():
            known.add(x)
            rounds[x], by[x], rule[x] = level, c, BITS
    present = [False] * n_wires
    for ms in merged:
        for m in ms:
            for s in m:
                present[s] = True
    status = [SEED if s in in_seed else DERIVED if s in known else OPEN if present[s] else ABSENT for s in range(n_wires)]
    return dict(status=status, round=[rounds.get(s, NONE) for s in range(n_wires)], by=[by.get(s, NONE) for s in range(n_wires)],
                rule=[rule.get(s, 0) for s in range(n_wires)], n_by_bits=sum(1 for k in rule.values() if k == BITS))


def summary(res):
    """(n_derived, n_absent, n_open, n_rounds, n_by_bits, ascending OPEN wires)"""
    return dr.summary(res["status"], res["round"])[:4] + (res["n_by_bits"], [s for s, k in enumerate(res["status"]) if k == OPEN])


class _Below:
    """the wires with a round below `level`, as a set to ask"""

    def __init__(self, rounds, level):
        self.rounds, self.level = rounds, level

    def __contains__(self, s):
        return self.rounds[s] != NONE and self.rounds[s] < self.level


def replay(circuit, w, seed, status, rounds, by, rule):
    """The certificate, checked on its own, wire by wire: by[x] names x and is not broken; a rule-1 wire is a PIN of it -- lin and
    quad are formed here again -- and every other wire of the row has a smaller round; a rule-2 wire's row qualifies -- (a), (b),
    (c), formed here again -- with respect to exactly the wires of smaller round.  Returns None, or what is wrong."""
    n_wires, rowsA, rowsB, rowsC = circuit
    if not (len(status) == len(rounds) == len(by) == len(rule) == n_wires):
        return "maps of the wrong length"
    held = held_wires(circuit, w)
    in_seed = set(seed) | {0}
    gives = {}                                                           # (constraint, level) -> the wires the row gives there
    for x in range(n_wires):
        if x in in_seed:
            if (status[x], rounds[x], by[x], rule[x]) != (SEED, 0, NONE, 0):
                return "seed wire %d is not reported as one" % x
            continue
        if status[x] != DERIVED:
            if status[x] == SEED or rounds[x] != NONE or by[x] != NONE or rule[x] != 0:
                return "wire %d is neither seed nor derived, yet has a round, a constraint or a rule" % x
            continue
        c = by[x]
        if rounds[x] == NONE or rounds[x] < 1 or c >= len(rowsA) or rule[x] not in (PIN, BITS):
            return "derived wire %d without a round, a constraint or a rule" % x
        ma, mb, mc = ms = tuple(ur.merged_row(r) for r in (rowsA[c], rowsB[c], rowsC[c]))
        wires = set(ma) | set(mb) | set(mc)
        if x not in wires:
            return "wire %d is not in constraint %d" % (x, c)
        a, b, cc = rb.values(rowsA, rowsB, rowsC, w, c)
        if (a * b - cc) % R:
            return "constraint %d is broken" % c
        if rule[x] == PIN:
            lin, quad = (ma.get(x, 0) * b + mb.get(x, 0) * a - mc.get(x, 0)) % R, ma.get(x, 0) * mb.get(x, 0) % R
            if (lin == 0) == (quad == 0):
                return "(%d, %d) is no PIN" % (x, c)
            for y in wires - {x}:
                if rounds[y] == NONE or rounds[y] >= rounds[x]:
                    return "wire %d of constraint %d is not known before round %d" % (y, c, rounds[x])
        else:
            if (c, rounds[x]) not in gives:
                gives[c, rounds[x]] = bit_row(ms, a, b, _Below(rounds, rounds[x]), held) or ()
            if x not in gives[c, rounds[x]]:
                return "constraint %d does not give wire %d with respect to the rounds below %d" % (c, x, rounds[x])
    return None


# ---------------------------------------------------------------- directed circuits
def seeded(case):
    """a solve_bits_reference case (its givens become the seed) as a case of this file"""
    circuit, w, header, given = case
    return circuit, w, header, list(given)


WIDTHS = (2, 63, 64, 65, 128, 129, 253)


@functools.lru_cache(maxsize=None)
def width(k, orient="A"):
    case, info = sb.width(k, orient)
    return seeded(case), info


def long_row(n_known=70):
    """a row of n_known + 4 incidences with all but 3 of them known: the gather takes several steps"""
    c = Circuit(9100 + n_known)
    known = [(c.wire(below(c.rng, R), True), 1 + below(c.rng, R - 1)) for _ in range(n_known)]
    x = c.wire(0b101 + sum(c.w[s] * kk for s, kk in known), True)
    bits = c.bits(3, 0b101)
    row = c.decomposition(bits, range(3), x, "A", 1, known=known)
    return seeded(c.case()), dict(bits=bits, row=row)


def coefficient_case(name):
    """4 bits of a seeded x; (case, info) with info["derives"]"""
    c = Circuit(sum(map(ord, name)) + 17)
    if name == "equal_coefficients":
        bits = c.bits(4, 0b1011)
        x = c.wire(c.w[bits[0]] + 2 * c.w[bits[1]] + 2 * c.w[bits[2]] + 8 * c.w[bits[3]], True)
        row = c.rows.mul([(bits[0], 1), (bits[1], 2), (bits[2], 2), (bits[3], 8)], const(1), v(x))
        return seeded(c.case()), dict(bits=bits, row=row, derives=False)
    top = {"exponent_252": 252, "coefficient_2_253": 253}[name]
    bits = c.bits(4, 0b1011)
    exps = [0, 1, 2, top]
    x = c.wire(sum(c.w[b] << e for b, e in zip(bits, exps)), True)
    row = c.decomposition(bits, exps, x)
    return seeded(c.case()), dict(bits=bits, row=row, derives=top <= MAX_EXP)


COEFFICIENTS = ("equal_coefficients", "exponent_252", "coefficient_2_253")


def unknown_case(name):
    """4 bits of a seeded x = 0b1011 under a witness that may break rows; (case, info) with info["derives"]: the wires the bit
    rule gives.  Every marking row of a wire has the residual quad b (b - 1): under one witness they are broken together or not
    at all, so "one marking row broken, another not" does not exist; the cases give a wire one row or two, in either state."""
    c = Circuit(sum(map(ord, name)) + 29)
    value, k = 0b1011, 4
    g = c.wire(7, True)
    w = None                                                                          # (the generating witness)
    if name == "not_boolean":
        bits = c.bits(k - 1, value & 7) + c.bits(1, 1, boolean=False)
        x = c.wire(value, True)
        row, derives = c.decomposition(bits, range(k), x), []
    elif name in ("marking_row_broken", "two_marking_rows_broken", "two_marking_rows_unbroken"):
        bits = c.bits(k, value)
        if name != "marking_row_broken":
            c.boolean(bits[1], "scaled")                                              # a second marking row of bits[1]
        x = c.wire(value, True)
        row = c.decomposition(bits, range(k), x)
        derives = bits if name == "two_marking_rows_unbroken" else []
        if name != "two_marking_rows_unbroken":                                       # bits[1] holds 2 and x the sum: the row itself holds
            w = list(c.w)
            w[bits[1]], w[x] = 2, 1 + 2 * 2 + 8
    elif name == "row_broken":
        bits = c.bits(k, value)
        x = c.wire(value, True)
        row, derives = c.decomposition(bits, range(k), x), []
        w = list(c.w)
        w[x] = value + 1
    elif name == "on_A_and_B":
        bits = c.bits(k, value)
        x = c.wire((c.w[bits[0]] + 2 * c.w[bits[1]] + g) * (c.w[bits[2]] + 2 * c.w[bits[3]] + g), True)
        row, derives = c.rows.mul([(bits[0], 1), (bits[1], 2), (0, g)], [(bits[2], 1), (bits[3], 2), (0, g)], v(x)), []
    elif name == "one_wire_on_both_sides":
        bits = c.bits(k, value)
        a = sum(c.w[b] << i for i, b in enumerate(bits))
        x = c.wire(a * (c.w[bits[0]] + 7), True)
        row, derives = c.rows.mul([(b, 1 << i) for i, b in enumerate(bits)], [(bits[0], 1), (0, 7)], v(x)), []
    elif name == "free_incidence":
        z = c.wire(0, True)                                                           # bits times a known 0: every lin_j = 0
        bits = c.bits(k, value)
        x = c.wire(0, True)
        row, derives = c.decomposition(bits, range(k), x, "Ag", g=z), []
    else:
        raise KeyError(name)
    circuit, w0, header, given = c.case()
    return (circuit, [t % R for t in (w if w is not None else w0)], header, list(given)), dict(bits=bits, row=row, derives=derives)


UNKNOWNS = ("not_boolean", "marking_row_broken", "two_marking_rows_broken", "two_marking_rows_unbroken", "row_broken", "on_A_and_B",
            "one_wire_on_both_sides", "free_incidence")


def pin_bits_pin():
    """x seeded -> its 5 bits (bit level, round 1) -> y = 3 b0 + b4 and z = y y (PIN, rounds 2 and 3) -> z's 6 bits (round 4):
    (case, {wire: (round, rule)})"""
    c = Circuit(4242)
    x = c.wire(0b10011, True)
    bits = c.bits(5, c.w[x])
    c.decomposition(bits, range(5), x, "C")
    y = c.wire(3 * c.w[bits[0]] + c.w[bits[4]])
    c.rows.mul([(bits[0], 3), (bits[4], 1)], const(1), v(y))
    z = c.wire(c.w[y] * c.w[y])
    c.rows.mul(v(y), v(y), v(z))
    more = c.bits(6, c.w[z])
    c.decomposition(more, range(6), z)
    want = {b: (1, BITS) for b in bits}
    want.update({y: (2, PIN), z: (3, PIN)})
    want.update({b: (4, BITS) for b in more})
    return seeded(c.case()), want


def pin_first():
    """s seeded -> x = s s (PIN, round 1) -> x's bits (round 2) -> y = b0 + b1 (PIN, round 3)"""
    c = Circuit(4243)
    s = c.wire(5, True)
    x = c.wire(25)
    c.rows.mul(v(s), v(s), v(x))
    bits = c.bits(5, 25)
    c.decomposition(bits, range(5), x)
    y = c.wire(c.w[bits[0]] + c.w[bits[1]])
    c.rows.mul([(bits[0], 1), (bits[1], 1)], const(1), v(y))
    want = {x: (1, PIN), y: (3, PIN)}
    want.update({b: (2, BITS) for b in bits})
    return seeded(c.case()), want


def falls_to_0_behind_bits():
    """determined_reference.falls_to_0 reached through the bit frontier: constraint 1, p = q, holds the two bits p and q of x
    outside; the bit level derives both, so in ONE expansion the row is listed when the first leaves and empty when the second
    has left.  Wire 1 is o with incidence 0 in o u = t, a PIN of a constraint with three wires outside: whoever reads the XOR of
    an EMPTY constraint as an incidence derives o.  (case, (o, u, t), (p, q))"""
    c = Circuit(4244)
    o, u, t = c.wire(5), c.wire(7), c.wire(35)
    c.rows.mul(v(o), v(u), v(t))                                                      # 0: all open
    x = c.wire(3, True)
    p, q = c.wire(1), c.wire(1)
    c.rows.mul(v(p), const(1), v(q))                                                  # 1: p = q, falls 2 -> 0
    c.boolean(p, "b(b-1)"), c.boolean(q, "bb=b")
    c.decomposition([p, q], range(2), x)
    return seeded(c.case()), (o, u, t), (p, q)


def conflict(n):
    """sb.conflict's n rows over the same seven bits, under the witness of row 0: the other rows are broken, so here a second
    set of n rows over the same bits with the SAME value stands behind them -- all unbroken, in one level: by is the lowest"""
    k = sb.CONFLICT_BITS
    c = Circuit(600 + n)
    value = 0b1010011
    junk = c.wire(3, True)
    c.rows.mul(v(junk), v(junk), const(9))                                            # constraint 0 is none of them
    bits = c.bits(k, value)
    row0 = len(c.rows.A)
    for i in range(n):
        lam = 1 + i
        x = c.wire(value, True)
        c.decomposition(bits, range(k), x, "ACB"[i % 3], lam)
    return seeded(c.case()), dict(bits=bits, row0=row0)


def partly_seeded(k=70, positions=(0, 5, 63, 64, 69), orient="C", lam=12345):
    case, info = sb.partly_given(k, list(positions), orient, lam)
    return seeded(case), info


EMPTY = {"no_constraints": (70, [], [], []),
         "no_incidences": (5, [[(0, 2)], [(0, 1)]], [[(0, 3)], [(0, 1)]], [[(0, 6)], [(0, 2)]])}


@functools.lru_cache(maxsize=None)
def generated(n, k=64):
    """section 10f's generated circuit (tools/bench_complete_bits.py; the same circuit at k = 64): n gadgets -- x seeded, its k
    bits, each with its own constraint in the four forms, ONE row sum 2^i b_i = x (orientation, scaling and exponent order vary
    by gadget), then y = sum a_i b_i and z = 3 y + x: two linear constraints behind the bits"""
    c = Circuit(0xBE7C)
    for i in range(n):
        x = c.wire(pm.SplitMix64(0x64B175 + i).next() & ((1 << k) - 1), True)
        bits = c.bits(k, c.w[x])
        exps = list(range(k)) if i % 4 else list(range(k - 1, -1, -1))               # every fourth: the LSB on the highest wire
        c.w[x] = sum(((c.w[x] >> j) & 1) << e for j, e in enumerate(exps))
        c.decomposition(bits, exps, x, ("A", "B", "C")[i % 3], 1 if i % 2 else 2 + below(c.rng, R - 2))
        coefs = [1 + (7 * j + i) % 5 for j in range(k)]
        y = c.wire(sum(a * c.w[b] for a, b in zip(coefs, bits)))
        c.rows.mul([(b, a) for a, b in zip(coefs, bits)], const(1), v(y))
        z = c.wire(3 * c.w[y] + c.w[x])
        c.rows.mul([(y, 3), (x, 1)], const(1), v(z))
    return seeded(c.case())


N_RANDOM = 40


@functools.lru_cache(maxsize=None)
def random_case(i):
    """solve_bits_reference's random circuit i under its generating assignment (the corrupted witnesses of the odd circuits and
    the gadgets with a wrong value break rows), its givens as the seed; in every second circuit about one BOOLEAN wire in five
    holds 2 or r - 1: its marking rows are broken, and so is every row that needs its value"""
    circuit, w, header, seed = seeded(sb.random_case(i))
    if i % 2 == 0:
        rng = pm.SplitMix64(0x4E1D0000 + i)
        w = [(2, R - 1)[rng.next() % 2] if mark and rng.next() % 5 == 0 else t for t, mark in zip(w, sb.boolean_wires(circuit))]
    return circuit, w, header, seed


@functools.lru_cache(maxsize=None)
def satisfying_case(i):
    """a small circuit with a SATISFYING witness: 1 .. 4 decompositions of at most 6 bits behind a PIN chain, in every
    orientation and exponent order, some bits seeded, now and then a bit without its constraint or a coefficient of 3"""
    c = Circuit(88000 + i)
    rng = c.rng
    s = c.wire(2 + below(rng, 50), True)
    t = c.wire(c.w[s] * c.w[s])
    c.rows.mul(v(s), v(s), v(t))
    for _ in range(1 + rng.next() % 4):
        k = 2 + rng.next() % 5
        value = below(rng, 1 << k)
        kind = rng.next() % 6
        exps = list(range(k))[::-1] if rng.next() % 3 == 0 else list(range(k))
        given = {j for j in range(k) if rng.next() % 8 == 0}
        bits = c.bits(k, value, given=given, boolean=kind != 2)
        if kind == 2:
            for b in bits[1:]:
                c.boolean(b)
        coefs = [(1 << e) if not (kind == 3 and j == 1) else 3 for j, e in enumerate(exps)]
        lam = 1 if rng.next() % 2 else 2 + below(rng, R - 2)
        orient = ("A", "B", "C", "Ag", "Bg")[rng.next() % 5]
        g = c.wire(below(rng, R) if rng.next() % 6 else 0, True) if orient[-1] == "g" else None
        total = sum(c.w[b] * kk for b, kk in zip(bits, coefs))
        x = c.wire(total * (c.w[g] if g is not None else 1), rng.next() % 6 != 0)
        side = [(b, lam * kk % R) for b, kk in zip(bits, coefs)]
        other = const(1) if g is None else v(g)
        if orient == "C":
            c.rows.mul(v(x, lam), const(1), side)
        elif orient[0] == "A":
            c.rows.mul(side, other, v(x, lam))
        else:
            c.rows.mul(other, side, v(x, lam))
        if kind >= 4:
            y = c.wire(sum(c.w[b] for b in bits))
            c.rows.mul([(b, 1) for b in bits], const(1), v(y))
    return seeded(c.case())


def unique_by_brute_force(circuit, w, known, c, out):
    """over all 0/1 assignments of the wires `out` of constraint c, every other wire as in w: how many satisfy c"""
    _, rowsA, rowsB, rowsC = circuit
    count, trial = 0, list(w)
    for values in itertools.product((0, 1), repeat=len(out)):
        for x, t in zip(out, values):
            trial[x] = t
        a, b, cc = rb.values(rowsA, rowsB, rowsC, trial, c)
        count += (a * b - cc) % R == 0
    return count
