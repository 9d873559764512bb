"""Big-integer reference of the unbound-wire scan (include/k16.h k16_r1cs_unbound_wires) and the circuits
its tests share.  Straight from the definition, in Python integers; it shares no code with the product.

Circuits are r1cs_builder's (n_wires, rowsA, rowsB, rowsC).  For wire i and constraint c the MERGED coefficients A^, B^, C^ are
the sums modulo r of the wire's terms in each combination; with a = A_c.w, b = B_c.w,
    lin = A^ b + B^ a - C^,   quad = A^ B^   (mod r)
and the wire is BOUND when some constraint has lin != 0 or quad != 0, ABSENT when all its merged coefficients are zero,
UNBOUND otherwise.  Wire 0 is the constant: BOUND."""
import functools

import pymodel as pm
import r1cs_builder as rb

R = pm.R
BOUND, ABSENT, UNBOUND = 0, 1, 2
EXTREMES = [0, 1, 2, R - 1, R - 2, (R - 1) // 2]


def merged_row(row):
    """{wire: sum of its coefficients mod r}, zero sums left out"""
    out = {}
    for s, k in row:
        out[s] = (out.get(s, 0) + k) % R
    return {s: k for s, k in out.items() if k}


def incidences(n_wires, rowsA, rowsB, rowsC):
    """[(wire, constraint, A^, B^, C^)] with a non-zero merged coefficient, by wire, then by constraint"""
    out = []
    for c, rows in enumerate(zip(rowsA, rowsB, rowsC)):
        ma, mb, mc = (merged_row(r) for r in rows)
        for s in set(ma) | set(mb) | set(mc):
            out.append((s, c, ma.get(s, 0), mb.get(s, 0), mc.get(s, 0)))
    return sorted(out)


def wire_constraints(n_wires, rowsA, rowsB, rowsC, wire):
    return [c for s, c, _, _, _ in incidences(n_wires, rowsA, rowsB, rowsC) if s == wire]


def classify(n_wires, rowsA, rowsB, rowsC, w):
    """The class of every wire under the assignment w (ints)."""
    a = [rb.dot(r, w) for r in rowsA]
    b = [rb.dot(r, w) for r in rowsB]
    present, bound = [False] * n_wires, [False] * n_wires
    for s, c, ka, kb, kc in incidences(n_wires, rowsA, rowsB, rowsC):
        present[s] = True
        if (ka * b[c] + kb * a[c] - kc) % R != 0 or ka * kb % R != 0:
            bound[s] = True
    return [BOUND if s == 0 or bound[s] else (UNBOUND if present[s] else ABSENT) for s in range(n_wires)]


def summary(classes):
    """(n_absent, n_unbound, ascending wires that are not BOUND, their classes) as k16_r1cs_unbound_wires reports them"""
    free = [s for s, k in enumerate(classes) if k != BOUND]
    return classes.count(ABSENT), classes.count(UNBOUND), free, [classes[s] for s in free]


# ---------------------------------------------------------------- directed circuits: (n_wires, rowsA, rowsB, rowsC, w)
def mux(sel):
    """sel (x - y) = out - y over wires 1 sel, 2 x, 3 y, 4 out"""
    x, y = 2, R - 2
    return 5, [[(1, 1)]], [[(2, 1), (3, R - 1)]], [[(4, 1), (3, R - 1)]], [1, sel, x, y, x if sel else y]


def square_at_zero():
    """x x = y at x = 0: lin = 0, quad = 1"""
    return 3, [[(1, 1)]], [[(1, 1)]], [[(2, 1)]], [1, 0, 0]


def tautology(k, x):
    """x (k one) = k x"""
    return 2, [[(1, 1)]], [[(0, k)]], [[(1, k)]], [1, x]


def cancellation(elsewhere, k=(R - 1) // 2):
    """wire 2 with k and r - k in one combination; `elsewhere`: also in a second constraint, w2 one = w3"""
    rowsA, rowsB, rowsC = [[(1, 1), (2, k), (2, R - k)]], [[(0, 2)]], [[(1, 2)]]
    if elsewhere:
        rowsA.append([(2, 1)]), rowsB.append([(0, 1)]), rowsC.append([(3, 1)])
    return 4, rowsA, rowsB, rowsC, [1, R - 1, 2, 2]


def zero_only_modulo_r(x=2):
    """(-x) (-one) = x with coefficients r - 1: lin = (r - 1)^2 - 1, a non-zero multiple of r"""
    return 2, [[(1, R - 1)]], [[(0, R - 1)]], [[(1, 1)]], [1, x]


COLUMN_CASES = [(n, at) for n in (1, 63, 64, 65, 129) for at in sorted({0, 63, 64, n - 1} & set(range(n))) + [None]]


def column(n, binding):
    """wire 1 in n constraints: tautologies w1 (2 one) = 2 w1, except constraint `binding` (None: none), w1 one = w2"""
    rowsA, rowsB, rowsC = [], [], []
    for c in range(n):
        rowsA.append([(1, 1)])
        rowsB.append([(0, 1)] if c == binding else [(0, 2)])
        rowsC.append([(2, 1)] if c == binding else [(1, 2)])
    return 3, rowsA, rowsB, rowsC, [1, R - 2, R - 2]


def pair_count(target, last_bound):
    """exactly `target` incidences, none of them on wire 0 (whose column the scan does not walk): constraint j is
    w_s w_t = 0 on the wires s = 1 + 2 j and t = s + 1, one of them 0 and the other not -- the zero one is bound (lin = the
    other's value), the other free (lin = 0) -- alternating; then single-incidence constraints up to the target, the LAST
    incidence on the highest wire: w w = 0 at 0 (bound by quad) or a lone A term (free)"""
    k = (target - 1) // 2
    rowsA = [[(1 + 2 * j, 1)] for j in range(k)]
    rowsB = [[(2 + 2 * j, 1)] for j in range(k)]
    rowsC = [[] for _ in range(k)]
    w = [1]
    for j in range(k):
        v = EXTREMES[1 + j % 5]
        w += [v, 0] if j & 1 else [0, v]
    for _ in range(target - 2 * k):                                # one or two single-incidence constraints
        s = len(w)
        rowsA.append([(s, 1)]), rowsB.append([(s, 1)] if last_bound else []), rowsC.append([])
        w.append(0)
    return len(w), rowsA, rowsB, rowsC, w


def word_edges(n_wires):
    """every wire bound (w one = 2 w at w = 0) except 63, 64, 127 and 128, which sit in tautologies"""
    free = {63, 64, 127, 128}
    rowsA = [[(s, 1)] for s in range(1, n_wires)]
    rowsB = [[(0, 1)] for _ in range(1, n_wires)]
    rowsC = [[(s, 1 if s in free else 2)] for s in range(1, n_wires)]
    return n_wires, rowsA, rowsB, rowsC, [1] + [R - 1 if s in free else 0 for s in range(1, n_wires)]


def unused_wires():
    """wire 3 and the highest wire, 5, are in no term"""
    return 6, [[(1, 1)], [(2, 1)]], [[(2, 1)], [(0, 1)]], [[(4, 1)], [(2, 1)]], [1, 2, R - 1, 0, R - 2, 0]


DIRECTED = {
    "mux_sel0": mux(0), "mux_sel1": mux(1), "square_at_zero": square_at_zero(),
    "cancellation_alone": cancellation(False), "cancellation_elsewhere": cancellation(True),
    "zero_only_modulo_r": zero_only_modulo_r(), "unused_wires": unused_wires(),
}
DIRECTED.update({"tautology_k%d_x%d" % (i, j): tautology(k, x) for i, k in enumerate(EXTREMES[1:]) for j, x in enumerate(EXTREMES)})
DIRECTED.update({"column_%d_%s" % (n, at): column(n, at) for n, at in COLUMN_CASES})
DIRECTED.update({"pairs_%d_%s" % (t, "bound" if lb else "free"): pair_count(t, lb) for t in (255, 256, 257) for lb in (False, True)})
DIRECTED.update({"wires_%d" % n: word_edges(n) for n in (64, 65, 128, 129)})


# ---------------------------------------------------------------- random circuits
N_RANDOM = 40


@functools.lru_cache(maxsize=None)
def random_circuit(seed):
    """(n_wires, rowsA, rowsB, rowsC, w, w_broken, planted): up to 200 wires, wires listed twice, coefficients that cancel, and
    three planted wires that appear nowhere else -- planted = (absent, tautology, mux input behind a zero selector).  w satisfies
    the circuit (the C side is solved through wire 0), w_broken does not."""
    rng = pm.SplitMix64(0x5EED0000 + seed)
    n_wires = 12 + rng.next() % 189                                   # 12 .. 200
    M = 4 + rng.next() % 60
    pool = list(range(1, n_wires))
    absent, taut, mux_x, sel = (pool.pop(rng.next() % len(pool)) for _ in range(4))
    coef = lambda: EXTREMES[1 + rng.next() % 5] if rng.next() % 4 == 0 else 1 + rng.below(R - 1)
    w = [1] + [(EXTREMES[rng.next() % 6] if rng.next() % 3 == 0 else rng.below(R)) for _ in range(n_wires - 1)]
    w[sel] = 0
    usable = pool + [0, sel]

    def row(n):
        r = [(usable[rng.next() % len(usable)], coef()) for _ in range(n)]
        if r and rng.next() % 3 == 0:
            r.append((r[0][0], coef()))                                # a wire listed twice
        if rng.next() % 4 == 0:
            s, k = usable[rng.next() % len(usable)], coef()
            r += [(s, k), (s, R - k)]                                  # ... and a pair that cancels
        return r

    rowsA, rowsB, rowsC = [], [], []
    for _ in range(M):
        a, b, c = row(rng.next() % 5), row(rng.next() % 4), row(rng.next() % 4)
        c.append((0, (rb.dot(a, w) * rb.dot(b, w) - rb.dot(c, w)) % R))
        rowsA.append(a), rowsB.append(b), rowsC.append(c)
    y, out, k = pool[rng.next() % len(pool)], pool[rng.next() % len(pool)], coef()
    plants = [([(taut, 1)], [(0, k)], [(taut, k)]),                                    # taut (k one) = k taut
              ([(sel, 1)], [(mux_x, 1), (y, R - 1)], [(0, 0)])]                        # sel (x - y) = 0 at sel = 0
    if seed & 1:
        plants.append(([(absent, k), (out, 1), (absent, R - k)], [(0, 1)], [(out, 1)]))   # absent only in terms that cancel
    for a, b, c in plants:
        at = rng.next() % (len(rowsA) + 1)
        rowsA.insert(at, a), rowsB.insert(at, b), rowsC.insert(at, c)
    assert rb.check(rowsA, rowsB, rowsC, w) == []
    for s in pool:
        w2 = list(w)
        w2[s] = (w2[s] + 1) % R
        if rb.check(rowsA, rowsB, rowsC, w2):
            return n_wires, rowsA, rowsB, rowsC, w, w2, (absent, taut, mux_x)
    raise AssertionError("no wire of circuit %d breaks a constraint" % seed)


# ---------------------------------------------------------------- one larger shape
@functools.lru_cache(maxsize=None)
def large_shape(n_bits=12000, n_bytes=3000, n_prod=5000, seed=7):
    """valid_key_builder.build()'s circuit recipe without the key: bit rows, then product rows c = (k1 a + k2 b) (k3 d)"""
    rng = pm.SplitMix64(seed)
    n_vars = 2 + n_bits + n_bytes + n_prod
    prod0 = 2 + n_bits + n_bytes
    prods = []
    for c in range(prod0, n_vars):
        a, b, d = 1 + rng.next() % (c - 1), 1 + rng.next() % (c - 1), 1 + rng.next() % (c - 1)
        prods.append((c, a, b, d, 1 + rng.next() % 1000, 1 + rng.next() % 1000, 1 + rng.next() % 1000))
    return dict(n_vars=n_vars, bit0=2, byte0=2 + n_bits, prod0=prod0, prods=prods)

