"""Big-integer reference of the witness completion (include/k16.h k16_r1cs_complete_witness) and the
circuits its tests share.  Straight from the definition, in Python integers; it shares no code with the product (merged
coefficients are unbound_reference.merged_row's).

A case is (circuit, w, header, given): circuit = r1cs_builder's (n_wires, rowsA, rowsB, rowsC), w an assignment (ints) of
which only the GIVEN positions and wire 0 are read, header = (nPubOut, nPubIn, nPrvIn), given a list of wires or None for the
header's inputs.

K_0 = given + {0}.  Level k: in constraint c exactly one wire x with a non-zero merged coefficient lies outside K_k; a0, b0, c0
are the sums of c's combinations over its wires in K_k; quad = A^ B^, lin = A^ b0 + B^ a0 - C^, k0 = a0 b0 - c0.  quad = 0 and
lin != 0: x joins K_k+1 with the value -k0 / lin, round[x] = k + 1, by[x] = the lowest such c."""
import functools

import determined_reference as dr
import pymodel as pm
import r1cs_builder as rb
import unbound_reference as ur
from determined_reference import Rows, const, v

R = pm.R
GIVEN, SOLVED, ABSENT, OPEN = 0, 1, 2, 3
NONE = 0xFFFFFFFF


def complete(circuit, w, given):
    """dict(status, round, by, wtns, failed, n_open_constraints) of the completion of w's given values"""
    n_wires, rowsA, rowsB, rowsC = circuit
    merged = [tuple(ur.merged_row(r) for r in rows) for rows in zip(rowsA, rowsB, rowsC)]
    in_given = set(given) | {0}
    val = {s: w[s] for s in in_given}
    assert val[0] == 1 and all(0 <= x < R for x in val.values()), "a given value the call refuses"
    rounds, by = {s: 0 for s in in_given}, {}
    part = lambda m, x: sum(k * val[s] for s, k in m.items() if s != x) % R     # the sum over the wires in K
    live, k = list(range(len(merged))), 0
    while True:
        new, still = {}, []
        for c in live:                                                 # ascending: the first c that gives x is the lowest
            ma, mb, mc = merged[c]
            outside = [s for s in set(ma) | set(mb) | set(mc) if s not in val]
            if not outside:
                continue
            still.append(c)
            if len(outside) != 1 or outside[0] in new:
                continue
            x = outside[0]
            ka, kb, kc = ma.get(x, 0), mb.get(x, 0), mc.get(x, 0)
            a0, b0, c0 = part(ma, x), part(mb, x), part(mc, x)
            quad, lin, k0 = ka * kb % R, (ka * b0 + kb * a0 - kc) % R, (a0 * b0 - c0) % R
            if quad == 0 and lin != 0:
                new[x] = (c, -k0 * pow(lin, R - 2, R) % R)
        if not new:
            break
        k += 1
        for x, (c, value) in new.items():
            rounds[x], by[x], val[x] = k, c, value
        live = still
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
                wtns=wtns, failed=[c for c in closed if c in broken], n_open_constraints=len(merged) - len(closed))


def summary(res):
    """(n_solved, n_absent, n_open, n_rounds, n_failed, n_open_constraints) as the call reports them"""
    st = res["status"]
    return (st.count(SOLVED), st.count(ABSENT), st.count(OPEN), max([0] + [k for k in res["round"] if k != NONE]),
            len(res["failed"]), res["n_open_constraints"])


def open_wires(res):
    return [s for s, k in enumerate(res["status"]) if k == OPEN]


def resolved(c):
    circuit, w, header, given = c
    return circuit, w, header, dr.default_seed(header) if given is None else given


# ---------------------------------------------------------------- directed circuits: the sides of the unknown
# wires 1 g1, 2 g2, 3 g3 given, 4 x unknown (unless said otherwise); EXPECTED: {wire: (status, round, by, value)}
def _sides():
    out, exp = {}, {}
    g1, g2, x = 2, 7, 5

    def one(name, a, b, c, w, want, given=(1, 2, 3)):
        rows = Rows()
        rows.mul(a, b, c)
        out[name] = (rows.circuit(len(w)), [t % R for t in w], (0, 0, 0), list(given))
        exp[name] = want

    solved = {4: (SOLVED, 1, 0, x)}
    one("x_on_A", v(4, 3) + v(1), v(2), v(3), [1, g1, g2, (3 * x + g1) * g2, x], solved)
    one("x_on_B", v(2), v(4, 3) + v(1), v(3), [1, g1, g2, (3 * x + g1) * g2, x], solved)
    one("x_on_C", v(1), v(2), v(4, 4) + v(3), [1, g1, g2, g1 * g2 - 4 * x, x], solved)
    one("x_on_A_and_C", v(4) + v(1), v(2), v(4, 2) + v(3), [1, g1, g2, (x + g1) * g2 - 2 * x, x], solved)       # lin = g2 - 2
    one("x_on_B_and_C", v(2), v(4) + v(1), v(4, 2) + v(3), [1, g1, g2, (x + g1) * g2 - 2 * x, x], solved)
    one("x_on_A_and_B", v(4) + v(1), v(4) + v(2), v(3), [1, g1, g2, (x + g1) * (x + g2), x], {4: (OPEN, NONE, NONE, 0)})
    one("lin_zero_A_b0_is_C", v(4), v(2), v(4, g2) + v(3), [1, g1, g2, 0, x], {4: (OPEN, NONE, NONE, 0)})         # x g2 = g2 x + 0
    one("lin_zero_k0_not", v(4), v(2), v(4, g2) + v(3), [1, g1, g2, 9, x], {4: (OPEN, NONE, NONE, 0)})            # unsatisfiable, unjudged
    one("k0_zero_value_zero", v(4), v(2), [], [1, g1, g2, 0, 0], {4: (SOLVED, 1, 0, 0)})                          # x g2 = 0
    one("given_0_and_r_minus_1", v(4) + v(1), v(2), v(3), [1, 0, R - 1, (x + 0) * (R - 1), x], solved)
    # (r - 1) x * (r - 1) one = x: lin = (r - 1)^2 - 1, a non-zero multiple of r
    n_wires, rowsA, rowsB, rowsC, w = ur.zero_only_modulo_r()
    out["lin_zero_only_modulo_r"], exp["lin_zero_only_modulo_r"] = ((n_wires, rowsA, rowsB, rowsC), w, (0, 0, 0), []), {1: (OPEN, NONE, NONE, 0)}
    # a solved 0 is known: x g2 = 0 gives x = 0, then y one = x + g1 gives y = g1 in round 2
    rows = Rows()
    rows.mul(v(5), const(1), v(4) + v(1))
    rows.mul(v(4), v(2), [])
    out["zero_is_a_value"] = (rows.circuit(6), [1, g1, g2, 0, 0, g1], (0, 0, 0), [1, 2, 3])
    exp["zero_is_a_value"] = {4: (SOLVED, 1, 1, 0), 5: (SOLVED, 2, 0, g1)}
    # the merged coefficient in the side table; a merged lin of 0; coefficients that cancel (determined_reference's circuit)
    out["merged_and_cancelling"] = dr.DIRECTED["merged_and_cancelling"]
    exp["merged_and_cancelling"] = {4: (SOLVED, 1, 0, 5), 5: (OPEN, NONE, NONE, 0), 6: (ABSENT, NONE, NONE, 0), 7: (SOLVED, 1, 2, 9)}
    return out, exp


SIDES, SIDES_EXPECTED = _sides()

SOLVE_SHORT = 16                       # csrc/r1cs_scan.hip: the terms of a candidate's three rows up to which one lane walks them
LONG_ROWS = sorted({SOLVE_SHORT - 3, SOLVE_SHORT - 2, SOLVE_SHORT - 1, SOLVE_SHORT, SOLVE_SHORT + 1, 63, 64, 65, 129})


def long_row(n, at):
    """(k_1 x_1 + .. + k_n x_n) s = y over wires 1 .. n, s = n + 1, y = n + 2 (n + 2 terms in the three rows); at None: y is the
    unknown, else x_(at + 1) inside the sum, with y given"""
    rng = pm.SplitMix64(0x10A60000 + 1000 * n + (999 if at is None else at))
    coef = lambda: ur.EXTREMES[1 + rng.next() % 5] if rng.next() % 3 == 0 else 1 + rng.below(R - 1)
    ks = [coef() for _ in range(n)]
    xs = [(ur.EXTREMES[rng.next() % 6] if rng.next() % 3 == 0 else rng.below(R)) for _ in range(n)]
    s = 1 + rng.below(R - 1)
    rows = Rows()
    rows.mul([(1 + i, ks[i]) for i in range(n)], v(n + 1), v(n + 2))
    w = [1] + xs + [s, sum(k * x for k, x in zip(ks, xs)) * s % R]
    unknown = n + 2 if at is None else 1 + at
    return rows.circuit(n + 3), w, (0, 0, 0), [i for i in range(1, n + 3) if i != unknown]


def conflict(n, lowest_last=False, deep=False):
    """n constraints x one = g_i claim ONE wire x with n different values in one round: by = constraint 0, the value g_0, the
    other n - 1 constraints fail.  lowest_last: the other wires' numbers are permuted -- x is the highest wire, its column ends
    the incidence list, and the g_i are numbered downwards: constraint 0's own wire is the last of them.  deep: the g_i are not
    given but solved in round 1 from s, so the claimants are listed by the expansion's atomics, in whatever order the launch runs"""
    if lowest_last:
        x, s, wires = n + 2, 1, list(range(n + 1, 1, -1))
    else:
        x, s, wires = 1, n + 2, list(range(2, n + 2))
    rows, w = Rows(), [0] * (n + 3)
    w[0], w[s] = 1, 3
    for i, g in enumerate(wires):
        w[g] = (11 + 5 * i) * (w[s] if deep else 1)
        rows.mul(v(x), const(1), v(g))
    for i, g in enumerate(wires if deep else []):
        rows.mul(v(s), const(11 + 5 * i), v(g))
    w[x] = w[wires[0]]
    return rows.circuit(n + 3), w, (0, 0, 0), [s] if deep else wires + [s]


CONFLICTS = [(n, last, deep) for n in (2, 64, 65, 257) for last, deep in ((False, False), (True, False), (False, True))]


@functools.lru_cache(maxsize=None)
def forward_circuit(i):
    """(case, depth): inputs given, then up to 300 gates, each defining ONE new wire on a random side of its constraint, with
    random and extreme coefficients; the other operands are earlier wires (every third circuit prefers the newest: deep chains).
    The witness is made gate by gate and satisfies the circuit; depth = the longest path of gates."""
    rng = pm.SplitMix64(0xF02D0000 + i)
    n_in, n_gates = 1 + rng.next() % 6, (300 if i % 5 == 0 else 1 + rng.next() % 300)
    coef = lambda: ur.EXTREMES[1 + rng.next() % 5] if rng.next() % 3 == 0 else 1 + rng.below(R - 1)
    w = [1] + [(ur.EXTREMES[rng.next() % 6] if rng.next() % 3 == 0 else rng.below(R)) for _ in range(n_in)]
    depth = [0] * (n_in + 1)
    rows = Rows()

    def pick():
        n = len(w)
        return n - 1 - rng.next() % min(n, 3) if i % 3 == 0 else rng.next() % n

    def lc():
        return [(pick(), coef()) for _ in range(1 + rng.next() % 3)]

    for _ in range(n_gates):
        z, k, side = len(w), coef(), rng.next() % 3
        a, b, c = lc(), lc(), lc()
        inv = lambda t: pow(t, R - 2, R)
        if side == 2:                                                  # a b = k z + c
            value = (rb.dot(a, w) * rb.dot(b, w) - rb.dot(c, w)) * inv(k) % R
            c = c + [(z, k)]
        else:                                                          # (k z + a) b = c, on A or on B
            if rb.dot(b, w) == 0:
                b = b + [(0, 1)]
            if rb.dot(b, w) == 0:
                b = [(0, 1)]
            b0 = rb.dot(b, w)
            value = (rb.dot(c, w) - rb.dot(a, w) * b0) * inv(k * b0 % R) % R
            a = a + [(z, k)]
            if side == 1:
                a, b = b, a
        used = {s for row in (a, b, c) for s in ur.merged_row(row) if s != z} | {0}         # (coefficients that cancel name no wire)
        depth.append(1 + max(depth[s] for s in used))
        w.append(value)
        rows.mul(a, b, c)
    assert rb.check(rows.A, rows.B, rows.C, w) == []
    return (rows.circuit(len(w)), w, (0, n_in, 0), None), max(depth)


N_FORWARD = 20
