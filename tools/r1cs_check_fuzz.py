"""Differential fuzz of the R1CS witness check against the Python reference checker (tests/r1cs_builder.py): random circuits
(constraints, wires, row lengths up to a few hundred terms, duplicate wires, coefficients from a mix of small and extreme
values), witnesses of the Keyless mix made to satisfy them, then random corruptions of wires and of C rows; count, ascending
list (under a random cap) and the A.w, B.w, C.w values of a failing and a passing row must agree.
python tools/r1cs_check_fuzz.py [cases] [seed]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "keyless-zk-proofs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import k16  # noqa: E402
import pymodel as pm  # noqa: E402
import r1cs_builder as rb  # noqa: E402

R = pm.R
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rs = np.random.RandomState(seed)
ctx = k16.Context(0)
EXTREME = [0, 1, 2, 255, 256, R - 1, R - 2, (R - 1) // 2, 1 << 253]


def value(full):
    u = rs.rand()
    if u < 0.15:
        return EXTREME[rs.randint(len(EXTREME))]
    if u < 0.15 + (0.25 if full else 0.75):
        return int(rs.randint(0, 256))
    return int.from_bytes(rs.bytes(32), "little") % R


bad, shapes, t0 = [], [], time.time()
for case in range(cases):
    M = int(rs.choice([1, 2, 63, 64, 65, 127, 128, 129, int(rs.randint(1, 700))]))
    n_wires = int(rs.randint(2, 400))
    w = [1] + [value(False) for _ in range(n_wires - 1)]
    nonzero = [i for i in range(n_wires) if w[i]]

    def row():
        n = int(rs.choice([0, 1, 2, 3, 63, 64, 65, int(rs.randint(0, 300))], p=[.1, .25, .2, .2, .05, .05, .05, .1]))
        return [(int(rs.randint(n_wires)), value(True)) for _ in range(n)]

    rowsA, rowsB, rowsC = [], [], []
    for c in range(M):
        a, b, cc = row(), row(), row()
        target = rb.dot(a, w) * rb.dot(b, w) % R
        s = nonzero[rs.randint(len(nonzero))]
        cc.append((s, (target - rb.dot(cc, w)) * pow(w[s], -1, R) % R))      # C is made to hold
        rowsA.append(a), rowsB.append(b), rowsC.append(cc)
    kind = int(rs.randint(4))
    w2, c2 = list(w), rowsC
    if kind == 1:                                                            # corrupt a few wires
        for _ in range(int(rs.randint(1, 4))):
            i = int(rs.randint(1, n_wires)) if n_wires > 1 else 0
            w2[i] = (w2[i] + 1 + int(rs.randint(3)) * (R - 2)) % R
    elif kind == 2:                                                          # C rows off by one, up or down
        hit = set(int(x) for x in rs.randint(0, M, size=rs.randint(1, 5)))
        c2 = [r + [(0, 1 if rs.rand() < .5 else R - 1)] if c in hit else r for c, r in enumerate(rowsC)]
    elif kind == 3:                                                          # a random witness: nearly everything fails
        w2 = [1] + [value(False) for _ in range(n_wires - 1)]
    want = rb.check(rowsA, rowsB, c2, w2)
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, c2))
    cap = int(rs.choice([0, 1, len(want), len(want) + 1, M]))
    n, idx = circ.check(rb.witness_bytes(w2), cap=cap)
    ok = n == len(want) and idx.tolist() == want[:cap]
    probe = ([want[0]] if want else []) + [c for c in range(M) if c not in set(want)][:1]
    for c in probe:
        ok = ok and circ.values(c) == rb.values(rowsA, rowsB, c2, w2, c)
    circ.close()
    shapes.append((M, n_wires, kind, len(want)))
    if not ok:
        bad.append(shapes[-1])
print(json.dumps({"fuzz": "k16_r1cs_check_mem vs the Python reference checker, random circuits and corruptions", "cases": cases,
                  "seed": seed, "mismatches": bad, "kinds": {str(k): sum(1 for s in shapes if s[2] == k) for k in range(4)},
                  "with_failures": sum(1 for s in shapes if s[3]), "max_constraints": max(s[0] for s in shapes),
                  "seconds": round(time.time() - t0, 1)}))
ctx.close()
sys.exit(1 if bad else 0)
