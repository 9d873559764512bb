"""Big-integer reference of the witness completion's bit rule (include/k16.h k16_r1cs_complete_witness_ex and
k16_r1cs_boolean_wires) and the circuits its tests share.  Straight from the definition, in Python
integers; the linear levels are solve_reference.complete's, run from the current set of known wires.

A case is (circuit, w, header, given) as in solve_reference; `given` is always a list here.

BOOLEAN: wire x >= 1, some constraint names (merged coefficient non-zero) no wire but x and wire 0 and, with A = a1 x + a0 and so
on, has quad = a1 b1 != 0, k = a0 b0 - c0 = 0, lin + quad = 0 (lin = a1 b0 + a0 b1 - c1).
THE BIT RULE with respect to K: constraint c, unknowns x_1 < .. < x_k outside K, 2 <= k <= 253; (a) all BOOLEAN; (b) A^ = 0 on
every unknown or B^ = 0 on every unknown; lin_j = A^_j b0 + B^_j a0 - C^_j, k0 = a0 b0 - c0; (c) lambda = lin of x_1, else of x_k
(0 is no lambda): every lin_j / lambda is 2^(e_j) as a canonical integer, e_j distinct, <= 252.  v = -k0 / lambda: v < 2^253 and
its set bits among the e_j -> FEASIBLE, x_j = bit e_j of v; else INFEASIBLE.
LEVELS: linear fixed point, ONE bit level (round = next number, by = the lowest feasible c naming x), linear again, until a bit
level solves nothing; the INFEASIBLE rows reported are that last level's."""
import functools

import determined_reference as dr
import pymodel as pm
import r1cs_builder as rb
import solve_reference as sr
import unbound_reference as ur
from determined_reference import Rows, const, v
from solve_reference import ABSENT, GIVEN, NONE, OPEN, SOLVED

R = pm.R
LINEAR, BITS = 1, 2
MAX_EXP = 252
inv = lambda t: pow(t, R - 2, R)
below = lambda rng, p: rng.below(1 << 254) % p        # (SplitMix64.below rejects on 254-bit draws: no use for a small p)


def merged_of(circuit):
    _, rowsA, rowsB, rowsC = circuit
    return [tuple(ur.merged_row(r) for r in rows) for rows in zip(rowsA, rowsB, rowsC)]


def boolean_form(ma, mb, mc):
    """the wire a constraint with these merged rows holds to {0, 1}, or None"""
    wires = (set(ma) | set(mb) | set(mc)) - {0}
    if len(wires) != 1:
        return None
    x = next(iter(wires))
    a1, b1, c1, a0, b0, c0 = ma.get(x, 0), mb.get(x, 0), mc.get(x, 0), ma.get(0, 0), mb.get(0, 0), mc.get(0, 0)
    quad, lin, k = a1 * b1 % R, (a1 * b0 + a0 * b1 - c1) % R, (a0 * b0 - c0) % R
    return x if quad != 0 and k == 0 and (lin + quad) % R == 0 else None


def boolean_wires(circuit):
    """[0 / 1 per wire]"""
    mark = [0] * circuit[0]
    for ms in merged_of(circuit):
        x = boolean_form(*ms)
        if x is not None:
            mark[x] = 1
    return mark


def bit_row(ms, val, booleans):
    """one constraint with respect to the known values val: None (the rule does not apply), ("feasible", {x: bit}) or
    ("infeasible", None)"""
    ma, mb, mc = ms
    out = sorted(s for s in set(ma) | set(mb) | set(mc) if s not in val)
    if not 2 <= len(out) <= MAX_EXP + 1:
        return None
    if not all(booleans[x] for x in out):
        return None                                                                  # (a)
    if any(x in ma for x in out) and any(x in mb for x in out):
        return None                                                                  # (b)
    part = lambda m: sum(k * val[s] for s, k in m.items() if s in val) % R
    a0, b0, c0 = part(ma), part(mb), part(mc)
    lins = [(ma.get(x, 0) * b0 + mb.get(x, 0) * a0 - mc.get(x, 0)) % R for x in out]
    k0 = (a0 * b0 - c0) % R
    for lam in (lins[0], lins[-1]):                                                  # (c)
        if lam == 0:
            continue
        ratios = [l * inv(lam) % R for l in lins]
        if any(t == 0 or t & (t - 1) or t.bit_length() - 1 > MAX_EXP for t in ratios):
            continue
        exps = [t.bit_length() - 1 for t in ratios]
        if len(set(exps)) != len(exps):
            continue
        value = -k0 * inv(lam) % R
        if value >> (MAX_EXP + 1) or value & ~sum(1 << e for e in exps):
            return "infeasible", None
        return "feasible", {x: (value >> e) & 1 for x, e in zip(out, exps)}
    return None


def complete(circuit, w, given, rules=LINEAR | BITS):
    """solve_reference.complete's dict plus rule (0 / 1 / 2 per wire), n_by_bits, infeasible (ascending)"""
    assert rules in (LINEAR, LINEAR | BITS)
    n_wires, rowsA, rowsB, rowsC = circuit
    merged = merged_of(circuit)
    booleans = boolean_wires(circuit)
    in_given = set(given) | {0}
    val = {s: w[s] for s in in_given}
    rounds, by, rule = {s: 0 for s in in_given}, {}, {}
    level, infeasible = 0, []
    while True:
        lin = sr.complete(circuit, [val.get(s, 0) for s in range(n_wires)], sorted(val))      # the linear rule from K
        depth = 0
        for s in range(n_wires):
            if lin["status"][s] == SOLVED:
                val[s], rounds[s], by[s], rule[s] = lin["wtns"][s], level + lin["round"][s], lin["by"][s], LINEAR
                depth = max(depth, lin["round"][s])
        level += depth
        if not rules & BITS:
            break
        new, infeasible = {}, []
        for c, ms in enumerate(merged):                                               # ascending: the first claim is the lowest
            res = bit_row(ms, val, booleans)
            if res is None:
                continue
            if res[0] == "infeasible":
                infeasible.append(c)
                continue
            for x, bit in res[1].items():
                new.setdefault(x, (c, bit))
        if not new:
            break
        level += 1
        for x, (c, bit) in new.items():
            val[x], rounds[x], by[x], rule[x] = bit, level, c, BITS
    present = [False] * n_wires
    for ms in merged:
        for m in ms:
            for s in m:
                present[s] = True
    status = [GIVEN if s in in_given else SOLVED if s in val else OPEN if present[s] else ABSENT for s in range(n_wires)]
    wtns = [val.get(s, 0) for s in range(n_wires)]
    closed = [c for c, ms in enumerate(merged) if all(s in val for m in ms for s in m)]
    broken = set(rb.check(rowsA, rowsB, rowsC, wtns))
    return dict(status=status, round=[rounds.get(s, NONE) for s in range(n_wires)], by=[by.get(s, NONE) for s in range(n_wires)],
                wtns=wtns, failed=[c for c in closed if c in broken], n_open_constraints=len(merged) - len(closed),
                rule=[rule.get(s, 0) for s in range(n_wires)], n_by_bits=sum(1 for k in rule.values() if k == BITS),
                infeasible=infeasible)


summary, open_wires = sr.summary, sr.open_wires


# ---------------------------------------------------------------- gadgets
BOOL_FORMS = ("b(b-1)", "b(1-b)", "bb=b", "scaled")


class Circuit:
    """a circuit under construction with its generating witness; wire 0 = 1"""

    def __init__(self, seed):
        self.rows, self.w, self.given, self.rng = Rows(), [1], [], pm.SplitMix64(0xB175000000 + seed)

    def wire(self, value, given=False):
        self.w.append(value % R)
        if given:
            self.given.append(len(self.w) - 1)
        return len(self.w) - 1

    def boolean(self, b, form=None):
        """b's own constraint, in one of the four forms"""
        form = BOOL_FORMS[self.rng.next() % 4] if form is None else form
        if form == "b(b-1)":
            return self.rows.mul(v(b), v(b) + const(-1), [])
        if form == "b(1-b)":
            return self.rows.mul(v(b), const(1) + v(b, -1), [])
        if form == "bb=b":
            return self.rows.mul(v(b), v(b), v(b))
        s, t = 1 + below(self.rng, R - 1), 1 + below(self.rng, R - 1)                   # (s b + 0) (t b - t) = 0
        return self.rows.mul(v(b, s), v(b, t) + const(-t), [])

    def bits(self, k, value, given=(), boolean=True):
        """k new wires holding the bits of value, LSB first, each with its own constraint; given: the positions that are given"""
        out = [self.wire((value >> i) & 1, i in given) for i in range(k)]
        for b in out:
            if boolean:
                self.boolean(b)
        return out

    def decomposition(self, bits, exps, x, orient="A", lam=1, known=(), g=None):
        """one row: lam (sum 2^exps[j] bits[j] + <known>) = lam x in the given orientation.  known: further (wire, coefficient)
        terms on the bits' side.  orient: "C" bits in C, "A" / "B" bits in A / B with the other side the constant 1, "Ag" / "Bg"
        with the other side the wire g and x the product.  Returns the constraint."""
        side = [(b, lam * (1 << e) % R) for b, e in zip(bits, exps)] + [(s, lam * k % R) for s, k in known]
        if orient == "C":
            return self.rows.mul(v(x, lam), const(1), side)
        other = const(1) if orient in ("A", "B") else v(g)
        return self.rows.mul(side, other, v(x, lam)) if orient[0] == "A" else self.rows.mul(other, side, v(x, lam))

    def case(self, satisfiable=True):
        circuit = self.rows.circuit(len(self.w))
        if satisfiable:
            assert rb.check(self.rows.A, self.rows.B, self.rows.C, self.w) == [], "the case's witness does not satisfy it"
        return circuit, list(self.w), (0, 0, 0), sorted(self.given)


def value_of(c, k):
    """a k-bit value with both end bits set and random bits between"""
    return (1 << (k - 1)) | 1 | below(c.rng, 1 << k) if k > 1 else 1


WIDTHS = (2, 3, 63, 64, 65, 128, 252, 253)


@functools.lru_cache(maxsize=None)
def width(k, orient="A"):
    """x given, k bits b_0 .. b_(k-1), sum 2^i b_i = x.  k = 254 needs exponent 253: refused.  k = 1 is the linear rule's."""
    c = Circuit(1000 + k)
    x = c.wire(value_of(c, k), True)
    bits = c.bits(k, c.w[x])
    row = c.decomposition(bits, range(k), x, orient)
    return c.case(), dict(x=x, bits=bits, row=row)


def oriented(name):
    """7 bits (wires 2 .. 8 or so) of x = 0b1011001 in the orientation `name`; returns (case, info); info["solved"]: does the rule fire"""
    c = Circuit(sum(map(ord, name)))
    k, value = 7, 0b1011001
    exps, lam, orient, g, solved = list(range(k)), 1, "A", None, True
    if name == "C":
        orient = "C"
    elif name == "A_times_known":
        orient, g = "Ag", c.wire(5 + below(c.rng, R - 5), True)
    elif name == "A_times_zero":
        orient, g, solved = "Ag", c.wire(0, True), False                              # lin_j = 0: nothing
    elif name == "B":
        orient = "B"
    elif name == "B_times_known":
        orient, g = "Bg", c.wire(5 + below(c.rng, R - 5), True)
    elif name == "scaled":
        lam = 2 + below(c.rng, R - 2)
    elif name == "scaled_C":
        orient, lam = "C", 2 + below(c.rng, R - 2)
    elif name == "lsb_on_highest_wire":
        exps = exps[::-1]                                                             # the second lambda
    elif name == "lsb_on_highest_wire_scaled":
        exps, lam = exps[::-1], 2 + below(c.rng, R - 2)
    elif name == "min_exponent_in_the_middle":
        exps, solved = [3, 2, 1, 0, 6, 5, 4], False                                   # neither end is the unit: refused by definition
    else:
        raise KeyError(name)
    total = sum(((value >> i) & 1) << e for i, e in enumerate(exps))
    x = c.wire(total * (c.w[g] if g is not None else 1), True)
    bits = c.bits(k, value)
    row = c.decomposition(bits, exps, x, orient, lam, g=g)
    return c.case(), dict(bits=bits, row=row, solved=solved, exps=exps, value=value)


ORIENTATIONS = ("C", "A_times_known", "A_times_zero", "B", "B_times_known", "scaled", "scaled_C", "lsb_on_highest_wire",
                "lsb_on_highest_wire_scaled", "min_exponent_in_the_middle")


def refusal(name):
    """4 bits; the row is no decomposition the rule takes: every bit stays OPEN.  (case, info)"""
    c = Circuit(sum(map(ord, name)))
    value, k = 0b1011, 4
    g = c.wire(7, True)
    if name == "coefficient_3":
        bits = c.bits(k, value)
        x = c.wire(c.w[bits[0]] + 3 * c.w[bits[1]] + 4 * c.w[bits[2]] + 8 * c.w[bits[3]], True)
        row = c.rows.mul([(bits[0], 1), (bits[1], 3), (bits[2], 4), (bits[3], 8)], const(1), v(x))
    elif name == "equal_exponents":
        bits = c.bits(k, value)
        x = c.wire(c.w[bits[0]] + 2 * c.w[bits[1]] + 2 * c.w[bits[2]] + 8 * c.w[bits[3]], True)
        row = c.rows.mul([(bits[0], 1), (bits[1], 2), (bits[2], 2), (bits[3], 8)], const(1), v(x))
    elif name == "one_unknown_not_boolean":
        bits = c.bits(k - 1, value & 7) + c.bits(1, 1, boolean=False)
        x = c.wire(value, True)
        row = c.decomposition(bits, range(k), x)
    elif name == "unknowns_on_A_and_B":
        bits = c.bits(k, value)
        x = c.wire((c.w[bits[0]] + 2 * c.w[bits[1]] + g) * (c.w[bits[2]] + 2 * c.w[bits[3]] + g), True)
        row = c.rows.mul([(bits[0], 1), (bits[1], 2), (0, g)], [(bits[2], 1), (bits[3], 2), (0, g)], v(x))
    elif name == "one_unknown_on_A_and_B":
        bits = c.bits(k, value)
        a = sum(c.w[b] << i for i, b in enumerate(bits))
        x = c.wire(a * (c.w[bits[0]] + 7), True)
        row = c.rows.mul([(b, 1 << i) for i, b in enumerate(bits)], [(bits[0], 1), (0, 7)], v(x))
    elif name == "254_bits":
        (case, info) = width(254)
        return case, dict(bits=info["bits"], row=info["row"])
    else:
        raise KeyError(name)
    return c.case(), dict(bits=bits, row=row)


REFUSALS = ("coefficient_3", "equal_exponents", "one_unknown_not_boolean", "unknowns_on_A_and_B", "one_unknown_on_A_and_B", "254_bits")


def partly_given(k, given_positions, orient="A", lam=1):
    c = Circuit(7000 + k)
    x = c.wire(value_of(c, k), True)
    bits = c.bits(k, c.w[x], given=set(given_positions))
    row = c.decomposition(bits, range(k), x, orient, lam)
    return c.case(), dict(bits=bits, row=row)


def infeasible_rows():
    """five decompositions of given values: 0 a bit outside the exponents {0, 1, 3}; 1 v >= 2^k; 2 v >= 2^253 (v = r - 1);
    3 a feasible one; 4 a scaled one whose v has a bit outside.  Rows 0, 1, 2, 4 are INFEASIBLE: (case, the rows, the feasible row)"""
    c = Circuit(66)
    rows = []
    x = c.wire(4, True)
    rows.append(c.decomposition(c.bits(3, 0), [0, 1, 3], x))
    x = c.wire(16 + 3, True)
    rows.append(c.decomposition(c.bits(4, 3), range(4), x, "C"))
    x = c.wire(R - 1, True)
    rows.append(c.decomposition(c.bits(5, 0), range(5), x, "B"))
    x = c.wire(0b10110, True)
    good_bits = c.bits(5, 0b10110)
    good = c.decomposition(good_bits, range(5), x)
    lam = 2 + below(c.rng, R - 2)
    x = c.wire(32, True)
    rows.append(c.decomposition(c.bits(3, 0), [0, 2, 4], x, "A", lam))
    return c.case(satisfiable=False), rows, good, good_bits


def long_row(n_known, k=64):
    """n_known given wires with random coefficients beside k unknown bits in one row"""
    c = Circuit(9000 + n_known)
    known = [(c.wire(below(c.rng, R), True), 1 + below(c.rng, R - 1)) for _ in range(n_known)]
    value = value_of(c, k)
    x = c.wire(value + sum(c.w[s] * kk for s, kk in known), True)
    bits = c.bits(k, value)
    row = c.decomposition(bits, range(k), x, "A", 1, known=known)
    return c.case(), dict(bits=bits, row=row)


def alternation(stages):
    """given x -> its bits -> y = a linear form of them -> y's bits -> ...: (case, [(kind, wires, round)] in the order solved)"""
    c = Circuit(300 + stages)
    k = 9
    x = c.wire(value_of(c, k), True)
    plan, rnd = [], 0
    for _ in range(stages):
        bits = c.bits(k, c.w[x])
        c.decomposition(bits, range(k), x, "C")
        rnd += 1
        plan.append((BITS, bits, rnd))
        coefs = [1 + below(c.rng, 5) for _ in bits]
        y = c.wire(sum(a * c.w[b] for a, b in zip(coefs, bits)))
        c.rows.mul([(b, a) for a, b in zip(coefs, bits)], const(1), v(y))
        rnd += 1
        plan.append((LINEAR, [y], rnd))
        x, k = y, 6                                                                   # y <= 5 * 9 < 2^6
    bits = c.bits(k, c.w[x])
    c.decomposition(bits, range(k), x)
    plan.append((BITS, bits, rnd + 1))
    return c.case(), plan


CONFLICT_BITS = 7


def conflict(n, lowest_last=False, behind=False):
    """n rows claim the SAME seven bit wires in one level, each with its own given value g_i (all different): by = the first of
    them, the value that of g_0, the other n - 1 rows close broken.  lowest_last: the bits are the highest wires and the g_i are
    numbered downwards, so that the winning row's own wire is the last of them.  behind: the winning row is NOT constraint 0 and
    not the first incidence of the bits' columns -- in front of the rows stand the bits' own constraints and a row over the
    same bits with a coefficient of 3 and an unknown sum y, which the rule refuses and the linear rule closes a round later.
    info["row0"]: the winning constraint."""
    k = CONFLICT_BITS
    c = Circuit(400 + n)
    gs = [(37 * i + 3) % 127 for i in range(n)]                                       # pairwise different below 2^7
    c.w += [0] * (n + k)
    if lowest_last:
        bits, wires = list(range(n + 1, n + k + 1)), list(range(n, 0, -1))
    else:
        bits, wires = list(range(1, k + 1)), list(range(k + 1, n + k + 1))
    for i, b in enumerate(bits):
        c.w[b] = (gs[0] >> i) & 1
    y = None
    if behind:
        for b in bits:
            c.boolean(b)
        y = c.wire(sum(c.w[b] * (3 if i == 1 else 1 << i) for i, b in enumerate(bits)))
        c.rows.mul([(b, 3 if i == 1 else 1 << i) for i, b in enumerate(bits)], const(1), v(y))
    row0 = len(c.rows.A)
    for g, s in zip(gs, wires):
        c.w[s] = g
        c.given.append(s)
        c.decomposition(bits, range(k), s, "AC"[len(c.rows.A) % 2])
    if not behind:
        for b in bits:
            c.boolean(b)
    return c.case(satisfiable=False), dict(bits=bits, value=gs[0], n_failed=n - 1, row0=row0, y=y)


CONFLICTS = [(n, last, behind) for n in (2, 64, 65) for last, behind in ((False, False), (True, False), (False, True), (True, True))]

N_RANDOM = 40


@functools.lru_cache(maxsize=None)
def random_case(i):
    """the closure's random circuit i (its satisfying or its corrupted witness, its seed as a list) with 1 .. 6 gadgets on new
    wires behind it: decompositions of a new given wire or of a wire of the circuit, in every orientation, scaled, in either
    exponent order, with given bits, a wrong value (infeasible), a coefficient that is no power of two, a bit without its
    constraint, and now and then a linear constraint over the bits that feeds a second decomposition"""
    circuit, w, header, seed = dr.resolved(dr.random_case(i))
    c = Circuit(50000 + i)
    c.rows.A, c.rows.B, c.rows.C = [list(r) for r in circuit[1]], [list(r) for r in circuit[2]], [list(r) for r in circuit[3]]
    c.w, c.given = list(w), list(seed)
    rng, n0 = c.rng, circuit[0]
    for _ in range(1 + rng.next() % 6):
        k = 2 + rng.next() % 11                                                       # 2 .. 12: brute force stays possible
        value = below(rng, 1 << k)
        kind = rng.next() % 8
        exps = list(range(k))
        if rng.next() % 3 == 0:
            exps = exps[::-1]
        if kind == 1:
            exps[rng.next() % k] += 1 + rng.next() % 3                                # a gap, or two equal exponents
        given = {j for j in range(k) if rng.next() % 8 == 0}
        bits = c.bits(k, value, given=given, boolean=kind != 2)
        if kind == 2:
            for b in bits[1:]:
                c.boolean(b)                                                          # bits[0] has no constraint of its own
        lam = 1 if rng.next() % 2 else 2 + below(rng, R - 2)
        orient = ("A", "B", "C", "Ag", "Bg")[rng.next() % 5]
        g = c.wire(below(rng, R) if rng.next() % 6 else 0, True) if orient[-1] == "g" else None
        pool = c.given if rng.next() % 4 else list(range(1, len(c.w)))                # known terms beside the bits; now and then any wire
        known = [(pool[rng.next() % len(pool)], below(rng, R)) for _ in range(rng.next() % 3)]
        known = [(s, kk) for s, kk in known if s not in bits]
        if kind == 3:
            known.append((bits[0], 2))                                                # a bit listed twice: coefficient 3 or 2^e + 2
        if rng.next() % 5 == 0:
            x = 1 + rng.next() % (n0 - 1)                                             # a wire of the circuit: any value, given or not
        else:                                                                         # the row's own value; kind 0: one bit too many
            total = sum(c.w[b] << e for b, e in zip(bits, exps)) + sum(kk * c.w[s] for s, kk in known) + (1 << k if kind == 0 else 0)
            x = c.wire(total * (c.w[g] if g is not None else 1), rng.next() % 8 != 0)
        c.decomposition(bits, exps, x, orient, lam, known=known, g=g)
        if kind >= 6:                                                                 # a linear constraint over the bits, decomposed again
            y = c.wire(sum(c.w[b] for b in bits))
            c.rows.mul([(b, 1) for b in bits], const(1), v(y))
            again = c.bits(4, c.w[y])
            c.decomposition(again, range(4), y, "C")
    return c.case(satisfiable=False)
