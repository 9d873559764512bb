"""The wide classes of the open-set solve (include/k16.h k16_r1cs_open_system_ex / k16_r1cs_open_direction_ex, DESIGN.md section
10i): a big-integer MODEL of the fraction-free elimination of k_r1cs_open_rref_wide, and the circuits its tests share.  The
definitions and the reference of every result are tests/open_system_reference.py's (osr.analyse takes the cap); nothing here
imports the product.

The model follows the kernel step by step over F_p, p a parameter:
    basis row b      reduced but not normalised: p_b != 0 in its own pivot column c_b, 0 in every other pivot column
    reduce a row     for the pivot columns among the row's own entries, in the order of the entries:
                     v <- p_b v - (o P) basis_b,  P <- P p_b      o: the ORIGINAL entry at c_b, P: the product of the p_b so far
    discard          the remainder is zero mod p in every non-pivot column
    insert           q: the lowest non-zero non-pivot column, s = v[q]; for the rows with basis_b[q] != 0:
                     basis_b <- s basis_b - basis_b[q] v; the remainder enters as it is"""
import functools

import open_system_reference as osr
import pymodel as pm
from open_system_reference import R, case, linear, product, values


def fraction_free(rows, n_cols, p):
    """rows: lists of (column, value) in the order of the entries, one entry a column; a value may be 0 mod p.  Returns (basis,
    pivots): basis[k] a dict {column: value != 0 mod p} of the k-th row IN THE ORDER OF INSERTION, pivots[k] its pivot column."""
    basis, pivots, rowof = [], [], {}
    for row in rows:
        v = {c: o % p for c, o in row}
        P = 1
        for c, o in row:
            if c not in rowof:
                continue
            b = basis[rowof[c]]
            pb, f = b[c], o * P % p
            v = {j: (pb * v.get(j, 0) - f * b.get(j, 0)) % p for j in set(v) | set(b)}
            P = P * pb % p
        live = [j for j, x in v.items() if x and j not in rowof]
        if not live:
            continue
        q = min(live)
        s = v[q]
        for k, b in enumerate(basis):
            f = b.get(q, 0)
            if f:
                basis[k] = {j: (s * b.get(j, 0) - f * v.get(j, 0)) % p for j in set(v) | set(b)}
        rowof[q] = len(basis)
        basis.append(v)
        pivots.append(q)
    return [{j: x for j, x in b.items() if x} for b in basis], pivots


def forced_of(basis, pivots):
    """the pivot columns whose row is zero in every non-pivot column"""
    ps = set(pivots)
    return {q for b, q in zip(basis, pivots) if all(j in ps for j in b)}


def normalised(basis, pivots, p):
    """{pivot column: the row divided by its pivot value}"""
    out = {}
    for b, q in zip(basis, pivots):
        inv = pow(b[q], p - 2, p)
        out[q] = {j: x * inv % p for j, x in b.items()}
    return out


def random_matrix(seed, p):
    """(rows, n_cols) over F_p: up to 2 x columns rows of mixed density, some a combination of earlier rows, some with an entry
    that is 0 mod p"""
    rng = pm.SplitMix64(0x0F1DE000 + seed)
    n_cols = 1 + rng.next() % 8
    rows = []
    for _ in range(rng.next() % (2 * n_cols + 1)):
        kind = rng.next() % 4
        if kind == 0 and len(rows) >= 2:                                   # forced to cancel: a combination of two earlier rows
            a, b = rows[rng.next() % len(rows)], rows[rng.next() % len(rows)]
            k0, k1 = rng.next() % p, rng.next() % p
            cols = sorted({c for c, _ in a} | {c for c, _ in b})
            row = [(c, (k0 * dict(a).get(c, 0) + k1 * dict(b).get(c, 0)) % p) for c in cols]
        else:
            density = 1 + rng.next() % 3
            row = [(c, rng.next() % p if rng.next() % 7 else 0) for c in range(n_cols) if rng.next() % 3 < density]
        rows.append(row)
    return rows, n_cols


# ---------------------------------------------------------------- circuits of the wide classes
CHAIN_SIZES = (65, 127, 128, 129, 255, 256)
DENSE = {"dense_128_full": (128, 128, 7), "dense_128_100": (128, 100, 8), "dense_256_40": (256, 40, 9), "dense_200_full": (200, 200, 10)}


@functools.lru_cache(maxsize=None)
def circuit(name):
    if name.startswith("chain_"):
        _, n, how = name.split("_")
        return osr.chain(int(n), how != "open", break_anchor=how == "broken")
    if name in DENSE:
        n, n_rows, seed = DENSE[name]
        return osr.dense_rows(n, n_rows, seed=seed)
    return {"redundant_100": redundant_wide, "cross_chain": cross_chain, "five_classes": five_classes, "more_than_slabs": more_than_slabs}[name]()


@functools.lru_cache(maxsize=None)
def result(name, max_wires=256):
    c = circuit(name)
    return osr.analyse(c["circuit"], c["w"], c["fixed"], max_wires=max_wires)


def redundant_wide(n=100, n_rows=12):
    """n wires, n_rows rows, all combinations of two dense rows with coefficients up to r - 1: rank 2, the other ten rows cancel
    only mod r"""
    w = values(n + 1, 41)
    rng = pm.SplitMix64(4141)
    base = [[1 + rng.below(R - 1) for _ in range(n)], [R - 1 - j for j in range(n)]]
    cons = []
    for _ in range(n_rows):
        k0, k1 = 1 + rng.below(R - 1), 1 + rng.below(R - 1)
        cons.append(linear([(1 + j, (k0 * base[0][j] + k1 * base[1][j]) % R or 1) for j in range(n)], w))
    return case(n + 1, cons, w)


def cross_chain(n=100):
    """a chain over wires 1 .. n anchored by x_1 + 2 x_n = s -- a row of two wires, so that the closure, which wants one
    constraint to pin a wire, derives nothing -- and x_1 x_2 = x_(n + 1): the chain is FORCED, the product's output UNDECIDED"""
    c = osr.chain(n, False)
    n_wires, rowsA, rowsB, rowsC = c["circuit"]
    w = c["w"] + [c["w"][1] * c["w"][2] % R]
    cons = [linear([(1, 1), (n, 2)], w), product(1, 2, n + 1)]
    return dict(circuit=(n_wires + 1, rowsA + [k[0] for k in cons], rowsB + [k[1] for k in cons], rowsC + [k[2] for k in cons]), w=w, fixed=[0])


def chains_side_by_side(sizes, seed, anchored, crossed=lambda i: False):
    n_wires = 1 + sum(sizes)
    w = values(n_wires, seed)
    cons, at = [], 1
    for i, size in enumerate(sizes):
        block = list(range(at, at + size))
        at += size
        for j in range(size - 1):
            cons.append(linear([(block[j], 1 + (i + j) % 3), (block[j + 1], 1)], w))
        if anchored(i):
            cons.append(linear([(block[-1], 3)], w))
        if crossed(i):
            cons.append(([(block[0], 1)], [(block[1], 1)], [(0, w[block[0]] * w[block[1]] % R)]))
    return case(n_wires, cons, w)


FIVE_SIZES = (3, 20, 50, 100, 250)


def five_classes(n_each=40):
    """components of 3, 20, 50, 100 and 250 wires, n_each of each, interleaved; three in four anchored, every fifth with a
    product row"""
    sizes = [FIVE_SIZES[i % 5] for i in range(5 * n_each)]
    return chains_side_by_side(sizes, 51, lambda i: (i // 5) % 4 != 1, lambda i: (i // 5) % 5 == 2)


ARENA_SLABS_256 = 64                                                        # csrc/r1cs_scan.hip OPEN_WIDE_ARENA / (256 * 9 * 256 * 4)


def more_than_slabs(extra=4):
    """ARENA_SLABS_256 + extra components of the 256-wire class: the first `extra` are anchored chains of 200 wires (rank 200),
    the last `extra` -- which the stride gives the same workgroups, so the same slabs -- open chains of 130 (rank 129)"""
    sizes = [200] * extra + [129 + i % 3 for i in range(ARENA_SLABS_256 - extra)] + [130] * extra
    return chains_side_by_side(sizes, 61, lambda i: i < extra or (extra <= i < ARENA_SLABS_256 and i % 2 == 0))


# ---------------------------------------------------------------- the wide random family
N_WIDE_RANDOM = 8


@functools.lru_cache(maxsize=None)
def wide_random_case(seed):
    """osr.random_case's blocks at the sizes of the wide classes: per block random sparse linear rows over neighbouring wires
    (sometimes more than the block has wires, sometimes too few), wires listed twice, sides swapped, in every other block a
    product row beside a row that pins one wire, now and then a broken row or a fixed wire"""
    rng = pm.SplitMix64(0x01DE0000 + seed)
    sizes = [66 + rng.next() % 60, 130 + rng.next() % 120, 2 + rng.next() % 40, 70 + rng.next() % 50, 140 + rng.next() % 100]
    n_wires = 1 + sum(sizes) + 2                                           # the last two wires: one in no term, one in a tautology
    w = values(n_wires, 700 + seed)
    cons, fixed, at = [], [], 1
    for k_block, size in enumerate(sizes):
        block = list(range(at, at + size))
        at += size
        n_rows = size - 3 + rng.next() % 6
        for k in range(n_rows):
            width = 2 + rng.next() % 3
            start = k % size
            terms = [(block[(start + j) % size], 1 + rng.below(R - 1) if rng.next() % 3 else 1 + rng.next() % 3) for j in range(width)]
            if rng.next() % 5 == 0:
                terms.append((terms[0][0], 1 + rng.below(R - 1)))          # a wire listed twice
            a, b, c = linear(terms, w)
            if rng.next() % 4 == 0:
                a, b = b, a                                                # B carries the row
            if rng.next() % 97 == 0:
                c = [(0, (c[0][1] + 1) % R)]                               # broken
            cons.append((a, b, c))
        if (k_block + seed) % 2 == 0:
            x, y, z = block[0], block[1], block[2]
            cons.append(([(x, 1)], [(y, 1)], [(z, 1), (0, (w[x] * w[y] - w[z]) % R)]))
            cons.append(linear([(block[size // 2], 5)], w))                # one wire pinned: FORCED beside the CROSS constraint
        if rng.next() % 3 == 0:
            fixed.append(block[rng.next() % size])
    t = n_wires - 1
    cons.append(([(t, 1)], [(0, 2)], [(t, 2)]))
    order = list(range(len(cons)))
    for i in range(len(order) - 1, 0, -1):
        j = rng.next() % (i + 1)
        order[i], order[j] = order[j], order[i]
    return case(n_wires, [cons[i] for i in order], w, fixed)


@functools.lru_cache(maxsize=None)
def wide_random_result(seed):
    c = wide_random_case(seed)
    return osr.analyse(c["circuit"], c["w"], c["fixed"], max_wires=256)
