"""Differential fuzz of the set-up from a trapdoor (k16_r1cs_setup): random circuits (tests/setup_reference.mixed: 1 .. 200
constraints, 0 .. 4 public wires split over outputs and inputs, rows of 0 .. 9 terms, wires listed twice, columns at the plan's
long-row boundary) and random trapdoors; the key must be byte-equal to the Python big-integer reference's with points from the
CPU oracle, the circuit must match it, a proof of the satisfying witness must verify and be byte-equal to the oracle's on the same
key, and a proof of a witness with one wire changed must be rejected.  python tools/setup_fuzz.py [cases] [seed]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "keyless-zk-proofs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import k16  # noqa: E402
import oracle_lib as ol  # noqa: E402
import pymodel as pm  # noqa: E402
import r1cs_builder as rb  # noqa: E402
import setup_reference as sr  # noqa: E402
import valid_key_builder as vkb  # noqa: E402

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
rs = np.random.RandomState(seed)
ctx = k16.Context(0)
d = tempfile.mkdtemp()
zk, wt = d + "/f.zkey", d + "/f.wtns"
bad, domains, t0 = [], set(), time.time()
for c in range(cases):
    M = int(rs.randint(1, 201))
    n_out, n_in = int(rs.randint(0, 3)), int(rs.randint(0, 3))
    circuit, w = sr.mixed(M, n_out, n_in, seed=seed * 100003 + c)
    n_wires, rowsA, rowsB, rowsC = circuit[:4]
    rng = pm.SplitMix64(seed * 7 + c)
    trapdoor = [1 + rng.below(pm.R - 1) for _ in range(5)]
    r, s = pm.limbs(rng.below(pm.R)), pm.limbs(rng.below(pm.R))
    circ = k16.R1cs(ctx, rb.write(n_wires, rowsA, rowsB, rowsC, n_pub_out=n_out, n_pub_in=n_in))
    zkey = circ.setup(trapdoor)
    why = []
    if zkey != sr.zkey(circuit, trapdoor, vkb.oracle_points):
        why.append("key differs from the reference's")
    if circ.match_zkey(zkey) != 0:
        why.append("circuit does not match its key")
    open(zk, "wb").write(zkey)
    wb = rb.witness_bytes(w)
    vkb.write_wtns(wt, wb)
    p, V = k16.Prover(ctx, zk), k16.VerifyingKey.from_zkey(ctx, zk)
    p.set_vk(V)
    js, proof, ok = p.prove_mem_verified(wb, r, s)
    if ok != 1:
        why.append("proof of the satisfying witness rejected")
    if js != ol.prove_files(zk, wt, r, s):
        why.append("proof differs from the oracle's")
    w2 = list(w)
    wire = n_out + n_in + 1 + int(rs.randint(0, n_wires - n_out - n_in - 2))
    w2[wire] = (w2[wire] + 1) % pm.R
    want = rb.check(rowsA, rowsB, rowsC, w2)
    js, proof, ok = p.prove_mem_verified(rb.witness_bytes(w2), r, s)
    n, got = circ.check_prover(p)
    if ok != (0 if want else 1) or got.tolist() != want:
        why.append("changed wire %d: ok=%d, check names %s, reference %s" % (wire, ok, got.tolist()[:4], want[:4]))
    p.close()
    V.close()
    circ.close()
    domains.add(sr.domain(M, n_out + n_in))
    if why:
        bad.append({"case": c, "M": M, "n_pub_out": n_out, "n_pub_in": n_in, "why": why})
print(json.dumps({"fuzz": "k16_r1cs_setup vs big-integer reference + oracle points, then prove + verify", "cases": cases,
                  "seed": seed, "mismatches": bad, "domains_seen": sorted(domains), "seconds": round(time.time() - t0, 1)}))
sys.exit(1 if bad else 0)
