"""Big-integer reference of the open-set solve (include/k16.h k16_r1cs_open_system / k16_r1cs_open_direction, DESIGN.md section
10h) and the circuits its tests share.  Straight from the definitions, in Python integers; it shares no code with the product.

Circuits are r1cs_builder's (n_wires, rowsA, rowsB, rowsC); w is an assignment (ints) and `fixed` a set of wires held fixed
(wire 0 always is).  Every function takes the prime p, so that the same code runs over a small field against brute force.

    outside wire       not fixed
    lin(x, c)          A^ b_c + B^ a_c - C^ (merged coefficients, sums of the assignment)
    dropped            a constraint the assignment breaks: no equation, no connectivity
    LINEAR / CROSS     an unbroken constraint with an outside incidence is LINEAR when its outside wires with A^ != 0 or those
                       with B^ != 0 are none, CROSS otherwise
    component          of the bipartite graph of outside wires and unbroken constraints; its id is its lowest wire; EXACT when
                       it has no CROSS constraint
    J                  rows: the component's LINEAR constraints, columns: its wires ascending, entries lin mod p
    FORCED             a pivot column of rref(J) whose row is zero in every non-pivot column"""
import functools

import pymodel as pm
import r1cs_builder as rb

R = pm.R
FIXED, ABSENT, FORCED, FREE, UNDECIDED, SKIPPED = 0, 1, 2, 3, 4, 5
NO_COMP = 0xFFFFFFFF
MAX_WIRES = 64
KIND_NONE, KIND_LINEAR, KIND_CROSS = 0, 1, 2


def merged(row, p):
    out = {}
    for s, k in row:
        out[s] = (out.get(s, 0) + k) % p
    return {s: k for s, k in out.items() if k}


def rref(rows, n_cols, p):
    """rows: dicts {column: value != 0}.  Returns (R, pivots): R[k] the k-th row of the reduced row echelon form as a dict,
    pivots[k] its pivot column, ascending."""
    basis = {}                                                     # pivot column -> row, kept reduced
    for row in rows:
        v = dict(row)
        for q, f in row.items():                                   # the factors are the row's own entries at the pivots
            if q in basis:
                for j, b in basis[q].items():
                    v[j] = (v.get(j, 0) - f * b) % p
        v = {j: x for j, x in v.items() if x}
        if not v:
            continue
        q = min(v)
        inv = pow(v[q], p - 2, p)
        v = {j: x * inv % p for j, x in v.items()}
        for b in basis.values():
            f = b.get(q, 0)
            if f:
                for j, x in v.items():
                    b[j] = (b.get(j, 0) - f * x) % p
                for j in [j for j, x in b.items() if not x]:
                    del b[j]
        basis[q] = v
    pivots = sorted(basis)
    return [basis[q] for q in pivots], pivots


def analyse(circuit, w, fixed, p=R, max_wires=MAX_WIRES):
    """Everything k16_r1cs_open_system reports, and per component what k16_r1cs_open_direction needs."""
    n_wires, rowsA, rowsB, rowsC = circuit
    fixed = set(fixed) | {0}
    M = len(rowsA)
    a = [sum(k * w[s] for s, k in r) % p for r in rowsA]
    b = [sum(k * w[s] for s, k in r) % p for r in rowsB]
    c = [sum(k * w[s] for s, k in r) % p for r in rowsC]
    broken = [a[i] * b[i] % p != c[i] for i in range(M)]
    present = [False] * n_wires
    parent = list(range(n_wires))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    kinds, lin_rows = [KIND_NONE] * M, {}
    for i in range(M):
        ma, mb, mc = merged(rowsA[i], p), merged(rowsB[i], p), merged(rowsC[i], p)
        wires = sorted(set(ma) | set(mb) | set(mc))
        for s in wires:
            present[s] = True
        out = [s for s in wires if s not in fixed]
        if broken[i] or not out:
            continue
        on_a, on_b = [s for s in out if s in ma], [s for s in out if s in mb]
        kinds[i] = KIND_CROSS if on_a and on_b else KIND_LINEAR
        for s in out[1:]:
            x, y = find(out[0]), find(s)
            parent[max(x, y)] = min(x, y)
        if kinds[i] == KIND_LINEAR:
            lin_rows[i] = {s: (ma.get(s, 0) * b[i] + mb.get(s, 0) * a[i] - mc.get(s, 0)) % p for s in out}
    classes, comp = [FIXED] * n_wires, [NO_COMP] * n_wires
    comps = {}
    for s in range(n_wires):
        if s in fixed:
            continue
        if not present[s]:
            classes[s] = ABSENT
            continue
        comp[s] = find(s)
        comps.setdefault(comp[s], dict(wires=[], rows=[], cross=0))["wires"].append(s)
    for i in range(M):
        if kinds[i] == KIND_NONE:
            continue
        first = min(s for s in set(merged(rowsA[i], p)) | set(merged(rowsB[i], p)) | set(merged(rowsC[i], p)) if s not in fixed)
        if kinds[i] == KIND_CROSS:
            comps[comp[first]]["cross"] += 1
        else:
            comps[comp[first]]["rows"].append(i)
    n_dims = 0
    for cid, k in comps.items():
        wires = k["wires"]
        k["exact"] = k["cross"] == 0
        if len(wires) > max_wires:
            k["skipped"] = True
            for s in wires:
                classes[s] = SKIPPED
            continue
        k["skipped"] = False
        col = {s: j for j, s in enumerate(wires)}
        J = [{col[s]: v for s, v in lin_rows[i].items() if v} for i in k["rows"]]
        k["R"], k["pivots"] = rref(J, len(wires), p)
        k["rank"] = len(k["pivots"])
        pivots = set(k["pivots"])
        forced = {q for row, q in zip(k["R"], k["pivots"]) if all(j in pivots for j in row)}
        for j, s in enumerate(wires):
            classes[s] = FORCED if j in forced else (FREE if k["exact"] else UNDECIDED)
        if k["exact"]:
            n_dims += len(wires) - k["rank"]
    listed = [s for s in range(n_wires) if classes[s] not in (FIXED, ABSENT)]
    return dict(classes=classes, comp=comp, comps=comps, kinds=kinds, lin_rows=lin_rows, broken=[i for i in range(M) if broken[i]],
                n_components=len(comps), n_dims=n_dims, listed=listed, n_forced=classes.count(FORCED), n_free=classes.count(FREE), n_undecided=classes.count(UNDECIDED),
                n_skipped=classes.count(SKIPPED), n_absent=classes.count(ABSENT), p=p)


def direction(res, wire):
    """The canonical direction of a FREE wire: {wire: value != 0}, d[wire] = 1.  {} for a wire that is not FREE."""
    p = res["p"]
    if res["classes"][wire] != FREE:
        return {}
    k = res["comps"][res["comp"][wire]]
    wires, pivots = k["wires"], k["pivots"]
    x = wires.index(wire)
    row_of = {q: row for row, q in zip(k["R"], pivots)}

    def v(f):
        out = {f: 1}
        for q, row in row_of.items():
            if row.get(f, 0):
                out[q] = (-row[f]) % p
        return out

    if x not in row_of:
        d = v(x)
    else:
        f = min(j for j in row_of[x] if j not in row_of)
        d = v(f)
        inv = pow(d[x], p - 2, p)
        d = {j: t * inv % p for j, t in d.items()}
    assert d[x] == 1
    return {wires[j]: t for j, t in sorted(d.items()) if t}


def moved(w, d, p=R):
    out = list(w)
    for s, t in d.items():
        out[s] = (out[s] + t) % p
    return out


def broken(circuit, w, p=R):
    _, rowsA, rowsB, rowsC = circuit
    dot = lambda row: sum(k * w[s] for s, k in row) % p
    return [i for i in range(len(rowsA)) if dot(rowsA[i]) * dot(rowsB[i]) % p != dot(rowsC[i])]


# ---------------------------------------------------------------- building blocks
def linear(terms, w, p=R):
    """sum k x = s as (A, B, C): the terms on A, one on B, s -- solved from w -- on C through wire 0"""
    return list(terms), [(0, 1)], [(0, sum(k * w[s] for s, k in terms) % p)]


def product(x, y, z):
    return [(x, 1)], [(y, 1)], [(z, 1)]


def circuit_of(n_wires, cons):
    return n_wires, [list(k[0]) for k in cons], [list(k[1]) for k in cons], [list(k[2]) for k in cons]


def case(n_wires, cons, w, fixed=()):
    return dict(circuit=circuit_of(n_wires, cons), w=list(w), fixed=sorted(set(fixed) | {0}))


def values(n, seed):
    rng = pm.SplitMix64(0x0BE50000 + seed)
    return [1] + [rng.below(R) for _ in range(n - 1)]


# ---------------------------------------------------------------- directed circuits
def two_by_two(rows, seed=1):
    """two linear rows over wires 1, 2"""
    w = values(3, seed)
    return case(3, [linear([(1, r[0]), (2, r[1])], w) for r in rows], w)


def selector(s):
    """s x = y over wires 1 s (fixed), 2 x, 3 y"""
    w = [1, s, 5, 5 * s % R]
    return case(4, [product(1, 2, 3)], w, fixed=[1])


def square(y_fixed=True):
    """x x = y over wires 1 x, 2 y"""
    return case(3, [product(1, 1, 2)], [1, 3, 9], fixed=[2] if y_fixed else [])


def product_with_sums(with_sums):
    """x y = z over wires 1, 2, 3; with x + y = s1 and x - y = s2"""
    w = [1, 11, 4, 44]
    cons = [product(1, 2, 3)]
    if with_sums:
        cons += [linear([(1, 1), (2, 1)], w), linear([(1, 1), (2, R - 1)], w)]
    return case(4, cons, w)


def chain(n, anchored, break_anchor=False, seed=3):
    """x_i + x_(i+1) = s_i over wires 1 .. n; anchored: and x_n = v.  break_anchor: the witness breaks that last row"""
    w = values(n + 1, seed)
    cons = [linear([(i, 1), (i + 1, 1)], w) for i in range(1, n)]
    if anchored:
        a, b, c = linear([(n, 1)], w)
        cons.append((a, b, [(0, (c[0][1] + 1) % R)]) if break_anchor else (a, b, c))
    return case(n + 1, cons, w)


def only_in_broken():
    """wire 1 only in a constraint the witness breaks; wires 2, 3 in a row that holds"""
    w = [1, 7, 8, 9]
    return case(4, [([(1, 1)], [(0, 1)], [(0, 6)]), linear([(2, 1), (3, 2)], w)], w)


def merged_terms():
    """row 0: wire 1 twice with k and r - k (no incidence) beside wire 2; row 1: wire 3 twice, 2 + 3 = 5, beside wire 2"""
    w = values(4, 9)
    k = (R - 1) // 2
    row0 = ([(1, k), (2, 3), (1, R - k)], [(0, 1)], [(0, 3 * w[2] % R)])
    row1 = linear([(3, 2), (2, 1), (3, 3)], w)
    return case(4, [row0, row1], w)


def redundant_rows(n_rows=12):
    """3 wires, n_rows rows, all combinations of two rows: rank 2"""
    w = values(4, 11)
    rng = pm.SplitMix64(77)
    base = [[1, 2, 3], [R - 1, 5, R - 2]]
    cons = []
    for _ in range(n_rows):
        k0, k1 = rng.below(R), rng.below(R)
        cons.append(linear([(1 + j, (k0 * base[0][j] + k1 * base[1][j]) % R) for j in range(3)], w))
    return case(4, cons, w)


def dense_rows(n=64, n_rows=3, seed=5):
    """n wires, n_rows rows with an entry in every column"""
    w = values(n + 1, seed)
    rng = pm.SplitMix64(1000 + seed)
    cons = [linear([(1 + j, 1 + rng.below(R - 1)) for j in range(n)], w) for _ in range(n_rows)]
    return case(n + 1, cons, w)


def permuted(c, seed=21):
    """the same circuit with its constraints in another order"""
    n_wires, rowsA, rowsB, rowsC = c["circuit"]
    order = list(range(len(rowsA)))
    rng = pm.SplitMix64(seed)
    for i in range(len(order) - 1, 0, -1):
        j = rng.next() % (i + 1)
        order[i], order[j] = order[j], order[i]
    return dict(circuit=(n_wires, [rowsA[i] for i in order], [rowsB[i] for i in order], [rowsC[i] for i in order]), w=c["w"],
                fixed=c["fixed"])


K_LARGE = pm.SplitMix64(4242).below(R - 2) + 2
DIRECTED = {
    "2x2_regular": two_by_two([(1, 1), (1, R - 1)]),
    "2x2_singular": two_by_two([(1, 2), (2, 4)]),
    "2x2_singular_mod_r": two_by_two([(R - 1, 2), ((R - 1) * (R - 1) % R, 2 * (R - 1) % R)]),
    "2x2_singular_large_k": two_by_two([(R - 1, R - 2), ((R - 1) * K_LARGE % R, (R - 2) * K_LARGE % R)]),
    "selector_0": selector(0), "selector_1": selector(1),
    "square_y_fixed": square(True), "square_open": square(False),
    "product_alone": product_with_sums(False), "product_with_sums": product_with_sums(True),
    "broken_anchor": chain(5, True, break_anchor=True), "only_in_broken": only_in_broken(),
    "merged_terms": merged_terms(),
    "redundant_rows": redundant_rows(), "dense_64": dense_rows(64, 3), "dense_64_full": dense_rows(64, 64, seed=6),
}
CHAIN_SIZES = (16, 17, 32, 33, 64)
for _n in CHAIN_SIZES + (65,):
    DIRECTED["chain_%d_anchored" % _n] = chain(_n, True)
    DIRECTED["chain_%d_open" % _n] = chain(_n, False)


# ---------------------------------------------------------------- the random family
N_RANDOM = 24


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """Blocks of wires of mixed sizes; inside a block random sparse linear rows (sometimes more than the block has wires,
    sometimes too few), some blocks with a product row, some rows broken, some wires fixed, wires listed twice."""
    rng = pm.SplitMix64(0x09E50000 + seed)
    sizes = [2 + rng.next() % 6 for _ in range(3 + rng.next() % 4)]
    if seed % 3 == 0:
        sizes.append(17 + rng.next() % 16)
    if seed % 4 == 1:
        sizes.append(33 + rng.next() % 32)
    n_wires = 1 + sum(sizes) + 2
    w = values(n_wires, 500 + seed)
    cons, fixed, at = [], [], 1
    for size in sizes:
        block = list(range(at, at + size))
        at += size
        n_rows = max(1, size - 2 + rng.next() % 4)
        for k in range(n_rows):
            width = 2 + rng.next() % 3
            start = k % size
            terms = [(block[(start + j) % size], 1 + rng.below(R - 1) if rng.next() % 3 else 1 + rng.next() % 3) for j in range(width)]
            if rng.next() % 5 == 0:
                terms.append((terms[0][0], 1 + rng.below(R - 1)))          # a wire listed twice
            a, b, c = linear(terms, w)
            if rng.next() % 4 == 0:                                        # the same row with the sides swapped: B carries it
                a, b = b, a
            if rng.next() % 13 == 0:
                c = [(0, (c[0][1] + 1) % R)]                               # broken
            cons.append((a, b, c))
        if rng.next() % 3 == 0 and size >= 3:
            x, y, z = block[0], block[1], block[2]
            cons.append(([(x, 1)], [(y, 1)], [(0, w[x] * w[y] % R)]) if rng.next() % 2 else
                        ([(x, 1)], [(y, 1)], [(z, 1), (0, (w[x] * w[y] - w[z]) % R)]))
        if rng.next() % 3 == 0:
            fixed.append(block[rng.next() % size])
    # the last two wires: one in no term, one in a tautology
    t = n_wires - 1
    cons.append(([(t, 1)], [(0, 2)], [(t, 2)]))
    order = list(range(len(cons)))
    for i in range(len(order) - 1, 0, -1):
        j = rng.next() % (i + 1)
        order[i], order[j] = order[j], order[i]
    return case(n_wires, [cons[i] for i in order], w, fixed)


@functools.lru_cache(maxsize=None)
def random_result(seed):
    c = random_case(seed)
    return analyse(c["circuit"], c["w"], c["fixed"])


@functools.lru_cache(maxsize=None)
def result(name):
    c = DIRECTED[name]
    return analyse(c["circuit"], c["w"], c["fixed"])


# ---------------------------------------------------------------- many components in one circuit
@functools.lru_cache(maxsize=None)
def many_components(n=1000):
    """n chains side by side: sizes of all three classes, most of them anchored, every seventh with a product row"""
    sizes = []
    for i in range(n):
        large, mid = i % 100 == 1 or i == 408, i % 20 == 3 or i % 200 == 8           # (most of them anchored below)
        sizes.append(33 + i % 31 if large else 17 + i % 16 if mid else 2 + i % 7)
    n_wires = 1 + sum(sizes)
    w = values(n_wires, 900)
    cons, at = [], 1
    for i, size in enumerate(sizes):
        block = list(range(at, at + size))
        at += size
        for j in range(size - 1):
            cons.append(linear([(block[j], 1 + (i + j) % 3), (block[j + 1], 1)], w))
        if i % 8 and i % 14 != 3:
            cons.append(linear([(block[-1], 3)], w))
        if i % 7 == 3 and size >= 2:
            cons.append(([(block[0], 1)], [(block[1], 1)], [(0, w[block[0]] * w[block[1]] % R)]))
    return case(n_wires, cons, w)


# ---------------------------------------------------------------- brute force over a small field
def small_random(seed, p=7):
    """(circuit, w, fixed) over F_p: 3 .. 6 wires, terms on all three sides, C solved through wire 0 (now and then not: broken)"""
    rng = pm.SplitMix64(0xB007 + seed)
    n_wires = 3 + rng.next() % 4
    M = 1 + rng.next() % 4
    w = [1] + [rng.next() % p for _ in range(n_wires - 1)]
    fixed = [s for s in range(1, n_wires) if rng.next() % 4 == 0]
    dot = lambda row: sum(k * w[s] for s, k in row) % p
    cons = []
    for _ in range(M):
        row = lambda n: [(rng.next() % n_wires, rng.next() % p) for _ in range(n)]
        a, b, c = row(1 + rng.next() % 3), row(rng.next() % 3), row(rng.next() % 3)
        if rng.next() % 3 == 0:
            b = [(0, 1 + rng.next() % (p - 1))]                            # a constant side: the row is linear
        c.append((0, (dot(a) * dot(b) - dot(c) + (1 if rng.next() % 9 == 0 else 0)) % p))
        cons.append((a, b, c))
    return circuit_of(n_wires, cons), w, fixed
