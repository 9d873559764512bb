"""Big-integer reference of the determinism closure (include/k16.h k16_r1cs_determined_wires), an
independent replayer of its certificates, and the circuits its tests share.  Straight from the definition, in Python integers;
it shares no code with the product (lin, quad and the kinds are second_value_reference's).

A case is (circuit, w, header, seed): circuit = r1cs_builder's (n_wires, rowsA, rowsB, rowsC), w the assignment (ints),
header = (nPubOut, nPubIn, nPrvIn) of the .r1cs file, seed a list of wires or None for the header's inputs.

The closure K is the least set with seed + {0} in it such that: constraint c is not broken by w, exactly one wire x with a
non-zero merged coefficient in c lies outside K, and (x, c) is a PIN  ==>  x in K.  Levels K_0 = seed + {0}, K_k+1 = K_k and
all x the rule gives with respect to K_k; round[x] = the first k with x in K_k, by[x] = the lowest c that gives x there."""
import functools

import pymodel as pm
import r1cs_builder as rb
import second_value_reference as sv
import unbound_reference as ur

R = pm.R
SEED, DERIVED, ABSENT, OPEN = 0, 1, 2, 3
NONE = 0xFFFFFFFF


def default_seed(header):
    n_pub_out, n_pub_in, n_prv_in = header
    return [0] + list(range(n_pub_out + 1, n_pub_out + 1 + n_pub_in + n_prv_in))


def constraint_kinds(circuit, w):
    """per constraint: {wire: FREE | PIN | ROOT} over the wires with a non-zero merged coefficient in it"""
    n_wires, rowsA, rowsB, rowsC = circuit
    a = [rb.dot(r, w) for r in rowsA]
    b = [rb.dot(r, w) for r in rowsB]
    out = [{} for _ in rowsA]
    for s, c, ka, kb, kc in ur.incidences(n_wires, rowsA, rowsB, rowsC):
        out[c][s] = sv.kind(ka, kb, kc, a[c], b[c])[0]
    return out


def closure(circuit, w, seed):
    """(status, round, by) of every wire, level by level"""
    n_wires, rowsA, rowsB, rowsC = circuit
    kinds = constraint_kinds(circuit, w)
    broken = set(rb.check(rowsA, rowsB, rowsC, w))
    in_seed = set(seed) | {0}
    known = set(in_seed)
    rounds, by = {s: 0 for s in known}, {}
    live = [c for c in range(len(rowsA)) if c not in broken]
    k = 0
    while True:
        new, still = {}, []
        for c in live:                                                 # ascending: the first c that gives x is the lowest
            outside = [s for s in kinds[c] if s not in known]
            if outside:
                still.append(c)
            if len(outside) == 1 and kinds[c][outside[0]] == sv.PIN:
                new.setdefault(outside[0], c)
        if not new:
            break
        k += 1
        for x, c in new.items():
            rounds[x], by[x] = k, c
        known |= set(new)
        live = still
    present = [False] * n_wires
    for c in kinds:
        for s in c:
            present[s] = True
    status = [SEED if s in in_seed else DERIVED if s in known else OPEN if present[s] else ABSENT for s in range(n_wires)]
    return status, [rounds.get(s, NONE) for s in range(n_wires)], [by.get(s, NONE) for s in range(n_wires)]


def summary(status, rounds):
    """(n_derived, n_absent, n_open, n_rounds, ascending OPEN wires) as k16_r1cs_determined_wires reports them"""
    return (status.count(DERIVED), status.count(ABSENT), status.count(OPEN), max([0] + [k for k in rounds if k != NONE]),
            [s for s, k in enumerate(status) if k == OPEN])


def replay(circuit, w, seed, status, rounds, by):
    """The certificate, checked on its own: going through the derived wires, by[x] is satisfied, (x, by[x]) is a PIN -- lin and
    quad are formed here again -- and every other wire of by[x] has a smaller round.  Returns None, or what is wrong."""
    n_wires, rowsA, rowsB, rowsC = circuit
    in_seed = set(seed) | {0}
    if not (len(status) == len(rounds) == len(by) == n_wires):
        return "maps of the wrong length"
    for x in sorted(range(n_wires), key=lambda s: (rounds[s], s)):
        if x in in_seed:
            if (status[x], rounds[x], by[x]) != (SEED, 0, NONE):
                return "seed wire %d is not reported as one" % x
            continue
        if status[x] != DERIVED:
            if status[x] == SEED or rounds[x] != NONE or by[x] != NONE:
                return "wire %d is neither seed nor derived, yet has a round or a constraint" % x
            continue
        c = by[x]
        if rounds[x] == NONE or rounds[x] < 1 or c >= len(rowsA):
            return "derived wire %d without a round or a constraint" % x
        ma, mb, mc = (ur.merged_row(r) for r in (rowsA[c], rowsB[c], rowsC[c]))
        wires = set(ma) | set(mb) | set(mc)
        if x not in wires:
            return "wire %d is not in constraint %d" % (x, c)
        a, b, cc = rb.values(rowsA, rowsB, rowsC, w, c)
        if (a * b - cc) % R:
            return "constraint %d is broken" % c
        lin, quad = (ma.get(x, 0) * b + mb.get(x, 0) * a - mc.get(x, 0)) % R, ma.get(x, 0) * mb.get(x, 0) % R
        if (lin == 0) == (quad == 0):
            return "(%d, %d) is no PIN" % (x, c)
        for y in wires - {x}:
            if rounds[y] == NONE or rounds[y] >= rounds[x]:
                return "wire %d of constraint %d is not known before round %d" % (y, c, rounds[x])
    return None


# ---------------------------------------------------------------- directed circuits
ONE = [(0, 1)]


def const(k):
    return [(0, k % R)]


class Rows:
    """constraints one after the other; mul(a, b, c) is <a, w> <b, w> = <c, w> with rows as lists of (wire, coefficient)"""

    def __init__(self):
        self.A, self.B, self.C = [], [], []

    def mul(self, a, b, c):
        self.A.append(list(a)), self.B.append(list(b)), self.C.append(list(c))
        return len(self.A) - 1

    def circuit(self, n_wires):
        return n_wires, self.A, self.B, self.C


def v(s, k=1):
    return [(s, k % R)]


def case(rows, w, header=None, seed=None):
    n_wires = len(w)
    header = header if header is not None else (0, 0, 0)
    assert rb.check(rows.A, rows.B, rows.C, w) == [], "the case's witness does not satisfy it"
    return rows.circuit(n_wires), [x % R for x in w], header, seed


def chain(depth):
    """x_1 given, x_i+1 = x_i x_i + 1: wire i + 1 in round i by constraint i - 1"""
    rows, w = Rows(), [1, 2]
    for i in range(1, depth + 1):
        rows.mul(v(i), v(i), v(i + 1) + const(-1))
        w.append((w[i] * w[i] + 1) % R)
    return case(rows, w, (0, 1, 0))


def diamond():
    """s = 1; a = 2 and b = 3 in round 1; d = 4 by the constraints 2 and 3 in round 2: by is 2"""
    rows, s = Rows(), 3
    rows.mul(v(1), v(1), v(2))
    rows.mul(v(1), v(1, 2), v(3))
    rows.mul(v(3), v(1), v(4))                                         # b s = d
    rows.mul(v(2, 2), v(1), v(4))                                      # 2 a s = d
    return case(rows, [1, s, s * s, 2 * s * s, 2 * s * s * s], (0, 1, 0))


def delayed():
    """x = 5 by constraint 5 in round 2 and by constraint 1 only in round 3 (its other wire b = 3 is round 2)"""
    rows, s = Rows(), 2
    a, b = s * s, s * s * s
    rows.mul(v(1), v(1), v(2))                                         # 0: a, round 1
    rows.mul(v(2), v(3, s), v(5, a))                                   # 1: a (s b) = a x with x = s b
    rows.mul(v(2), v(1), v(3))                                         # 2: b = a s, round 2
    rows.mul(v(1), v(1), v(4))                                         # 3: filler, wire 4
    rows.mul(v(1), v(1), v(6))                                         # 4: filler, wire 6
    rows.mul(v(2), v(1, s), v(5))                                      # 5: x = a s^2, round 2
    return case(rows, [1, s, a, b, s * s, s * b, s * s], (0, 1, 0))


def falls_3_to_1():
    """constraint 3 holds p, q and x outside; p and q both come in round 1, so it falls 3 -> 1 in ONE expansion and gives x"""
    rows, s = Rows(), 3
    rows.mul(v(1), v(1), v(2))                                         # p
    rows.mul(v(1), v(1, 2), v(3))                                      # q
    rows.mul(v(1), v(1), v(5))                                         # (another wire of round 1)
    rows.mul(v(2) + v(3), v(1), v(4))                                  # (p + q) s = x
    return case(rows, [1, s, s * s, 2 * s * s, 3 * s * s * s, s * s], (0, 1, 0))


def falls_to_0():
    """constraint 3, p s = q, holds p and q outside, both of round 1: it is listed when the first leaves and empty when the
    second has left.  Wire 1 is o with incidence 0 in o u = t, a PIN of a constraint with three wires outside: whoever reads the
    XOR of an EMPTY constraint as an incidence derives o"""
    rows, s = Rows(), 3
    rows.mul(v(1), v(2), v(3))                                         # 0: o u = t, all open
    rows.mul(v(4), v(4), v(5))                                         # 1: p = s s
    rows.mul(v(4), v(4, s), v(6))                                      # 2: q = s^3
    rows.mul(v(5), v(4), v(6))                                         # 3: p s = q
    return case(rows, [1, 5, 7, 35, s, s * s, s * s * s], (3, 1, 0))


def moving_pair(seed=None):
    """wires 1 out, 2 in, 3 tmp; out = tmp tmp, both hints: they move together"""
    rows = Rows()
    rows.mul(v(3), v(3), v(1))
    return case(rows, [1, 49, 5, 7], (1, 1, 0), seed)


def square_root(r):
    """wires 1 x (input), 2 r: r r = x"""
    rows = Rows()
    rows.mul(v(2), v(2), v(1))
    return case(rows, [1, r * r, r], (0, 1, 0))


def mux(sel, seed):
    n_wires, rowsA, rowsB, rowsC, w = ur.mux(sel)
    return (n_wires, rowsA, rowsB, rowsC), w, (0, 3, 0), seed


def free_but_counted():
    """constraint 0: p z = q at z = 0 holds p (FREE: lin = z = 0) and q (PIN) outside: q must wait for p, which comes in
    round 2 -- q is round 3.  Constraint 3 is the same with p2, which nothing else names: q2 stays OPEN"""
    rows, s = Rows(), 2
    # wires 1 s, 2 z, 3 a, 4 p, 5 q, 6 p2, 7 q2
    rows.mul(v(4), v(2), v(5))                                         # 0: p z = q
    rows.mul(v(1), v(1), v(3))                                         # 1: a = s s
    rows.mul(v(3), v(1), v(4))                                         # 2: p = a s
    rows.mul(v(6), v(2), v(7))                                         # 3: p2 z = q2
    return case(rows, [1, s, 0, s * s, s * s * s, 0, 11, 0], (0, 2, 0))


def broken_link(corrupt):
    """a = s s, b = a s, e = s s; corrupt: b is off, constraint 1 alone fails and b, which only it could give, is OPEN"""
    rows, s = Rows(), 3
    rows.mul(v(1), v(1), v(2))
    rows.mul(v(2), v(1), v(3))
    rows.mul(v(1), v(1), v(4))
    circuit, w, header, seed = case(rows, [1, s, s * s, s * s * s, s * s], (0, 1, 0))
    if corrupt:
        w[3] = (w[3] + 1) % R
        assert rb.check(rows.A, rows.B, rows.C, w) == [1]
    return circuit, w, header, seed


def merged_and_cancelling():
    """wires 1 s, 2 y, 3 y2, 4 x, 5 x2, 6 z, 7 y3.  Seed s, y, y2.
    0: (k1 x + k2 x) s = y with k1 + k2 = 2: the merged A^ = 2 is in the side table, lin = 2 s: x is derived
    1: (k1 x2 + k2 x2) s = 2 s x2 + y2 - 2 s x2: lin = 2 s - 2 s = 0 with the MERGED coefficient (k1 alone would pin): x2 OPEN
    2: (k z - k z + s) s = y3: z's coefficients cancel, z is no incidence, ABSENT, and does not keep y3 from being derived"""
    rows, s, x, x2 = Rows(), 3, 5, 7
    k1, k2 = R - 5, 7
    rows.mul(v(4, k1) + v(4, k2), v(1), v(2))
    rows.mul(v(5, k1) + v(5, k2), v(1), v(5, 2 * s) + v(3))
    rows.mul(v(6, 9) + v(6, -9) + v(1), v(1), v(7))
    w = [1, s, 2 * x * s, 0, x, x2, 123, s * s]
    return case(rows, w, (0, 0, 0), [1, 2, 3])


def wide(n):
    """s s = a_i for n wires: n first candidates, a frontier of n in round 1; 2 n incidences, none on wire 0"""
    rows, s = Rows(), 3
    for i in range(n):
        rows.mul(v(1), v(1, 1 + i), v(2 + i))
    return case(rows, [1, s] + [(1 + i) * s * s for i in range(n)], (0, 1, 0))


def fan(n):
    """a = s s, then a s = b_i for n wires: a's column has n + 1 incidences, walked when a is expanded; that expansion lists n
    candidates and round 2 has a frontier of n"""
    rows, s = Rows(), 2
    rows.mul(v(1), v(1), v(2))
    for i in range(n):
        rows.mul(v(2), v(1, 1 + i), v(3 + i))
    return case(rows, [1, s, s * s] + [(1 + i) * s ** 3 for i in range(n)], (0, 1, 0))


def seventy():
    """one constraint with 70 wires, 69 of them seeded: (x_1 + .. + x_68) s = y"""
    rows = Rows()
    xs = list(range(1, 69))
    rows.mul([(i, 1) for i in xs], v(69), v(70))
    w = [1] + [i + 1 for i in xs] + [3]
    w.append(sum(w[1:69]) * 3)
    return case(rows, w, (0, 69, 0))


DIRECTED = {
    "chain_300": chain(300), "chain_3": chain(3), "diamond": diamond(), "delayed": delayed(), "falls_3_to_1": falls_3_to_1(),
    "falls_to_0": falls_to_0(), "moving_pair": moving_pair(), "moving_pair_tmp_seeded": moving_pair([3]),
    "square_root_at_3": square_root(3), "square_root_at_0": square_root(0),
    "mux_sel0_x": mux(0, [1, 3, 4]), "mux_sel1_x": mux(1, [1, 3, 4]), "mux_sel0_out": mux(0, [1, 2, 3]), "mux_sel1_out": mux(1, [1, 2, 3]),
    "mux_sel0_default": mux(0, None), "free_but_counted": free_but_counted(),
    "broken_link": broken_link(True), "repaired_link": broken_link(False), "merged_and_cancelling": merged_and_cancelling(),
    "seventy": seventy(),
}
DIRECTED.update({"wide_%d" % n: wide(n) for n in (63, 64, 65, 255, 256, 257)})
DIRECTED.update({"fan_%d" % n: fan(n) for n in (62, 63, 64, 255, 256, 257)})     # columns of 63, 64, 65, 256, 257, 258

# what some of them must give, by hand: {wire: (status, round, by)}
EXPECTED = {
    "chain_3": {1: (SEED, 0, NONE), 2: (DERIVED, 1, 0), 3: (DERIVED, 2, 1), 4: (DERIVED, 3, 2)},
    "diamond": {2: (DERIVED, 1, 0), 3: (DERIVED, 1, 1), 4: (DERIVED, 2, 2)},
    "delayed": {2: (DERIVED, 1, 0), 3: (DERIVED, 2, 2), 5: (DERIVED, 2, 5), 4: (DERIVED, 1, 3), 6: (DERIVED, 1, 4)},
    "falls_3_to_1": {2: (DERIVED, 1, 0), 3: (DERIVED, 1, 1), 4: (DERIVED, 2, 3)},
    "falls_to_0": {1: (OPEN, NONE, NONE), 2: (OPEN, NONE, NONE), 3: (OPEN, NONE, NONE), 5: (DERIVED, 1, 1), 6: (DERIVED, 1, 2)},
    "moving_pair": {1: (OPEN, NONE, NONE), 2: (SEED, 0, NONE), 3: (OPEN, NONE, NONE)},
    "moving_pair_tmp_seeded": {1: (DERIVED, 1, 0), 2: (ABSENT, NONE, NONE), 3: (SEED, 0, NONE)},
    "square_root_at_3": {2: (OPEN, NONE, NONE)}, "square_root_at_0": {2: (DERIVED, 1, 0)},
    "mux_sel0_x": {2: (OPEN, NONE, NONE)}, "mux_sel1_x": {2: (DERIVED, 1, 0)},
    "mux_sel0_out": {4: (DERIVED, 1, 0)}, "mux_sel1_out": {4: (DERIVED, 1, 0)},
    "mux_sel0_default": {1: (SEED, 0, NONE), 2: (SEED, 0, NONE), 3: (SEED, 0, NONE), 4: (DERIVED, 1, 0)},
    "free_but_counted": {3: (DERIVED, 1, 1), 4: (DERIVED, 2, 2), 5: (DERIVED, 3, 0), 6: (OPEN, NONE, NONE), 7: (OPEN, NONE, NONE)},
    "broken_link": {2: (DERIVED, 1, 0), 3: (OPEN, NONE, NONE), 4: (DERIVED, 1, 2)},
    "repaired_link": {2: (DERIVED, 1, 0), 3: (DERIVED, 2, 1), 4: (DERIVED, 1, 2)},
    "merged_and_cancelling": {4: (DERIVED, 1, 0), 5: (OPEN, NONE, NONE), 6: (ABSENT, NONE, NONE), 7: (DERIVED, 1, 2)},
    "seventy": {70: (DERIVED, 1, 0)},
}


def resolved(c):
    """(circuit, w, header, the seed as a list) of a case"""
    circuit, w, header, seed = c
    return circuit, w, header, default_seed(header) if seed is None else seed


# ---------------------------------------------------------------- random circuits
N_RANDOM = 40


@functools.lru_cache(maxsize=None)
def random_case(i):
    """unbound_reference's random circuit i with the satisfying witness (even i) or the corrupted one (odd i), and either a
    header whose inputs are the first 70 % of the wires (i % 4 < 2: the default seed) or a random 70 % of them as a list"""
    n_wires, rowsA, rowsB, rowsC, w, w_broken, _ = ur.random_circuit(i)
    rng = pm.SplitMix64(0xDE7E0000 + i)
    n_in = (n_wires - 1) * 7 // 10
    if i % 4 < 2:
        header, seed = (0, n_in // 2, n_in - n_in // 2), None
    else:
        pool = list(range(1, n_wires))
        header, seed = (0, 0, 0), sorted(pool.pop(rng.next() % len(pool)) for _ in range(n_in))
    return (n_wires, rowsA, rowsB, rowsC), (w_broken if i & 1 else w), header, seed
