"""The unbound-wire scan (k16_r1cs_unbound_wires) beside the check whose sums it reads (k16_r1cs_check_prover_witness), same
process, alternating call by call.
    python tools/bench_unbound.py [--runs 5] [--calls 50] [--warmup 5] [--scale 1.0] [--out FILE.json]
Circuit: the SYNTHETIC circuit of the Keyless shape (tests/valid_key_builder.py: nVars 1,343,588, 1,236,099 constraints, one
public input) as an .r1cs file from the builder's `shape` (tests/r1cs_builder.py write_from_shape), sized as tools/bench_setup.py
sizes it; the key comes from the set-up on the device (k16_r1cs_setup).  Its rows hold 1-2 terms: the real Keyless circuit's
columns are longer, so these timings and class counts are the synthetic circuit's, not the real circuit's.  Recorded:
    first    the first k16_r1cs_unbound_wires of an object: the incidence list is built on the host and uploaded, then the scan
    scan     every later call: one launch over the incidences, the mask's download, the host's pass over it
    check    k16_r1cs_check_prover_witness just before each scan -- the witness of the last prove, read in place
with the number of incidences (all, and those of the wires 1 .. nWires - 1, which the scan walks), the device bytes the scan added (hipMemGetInfo around the first call) and the wires per class,
which are asserted against the big-integer reference of tests/unbound_reference.py.  Every call is timed around its C entry
point and ends in a device synchronise of its own; p50 / p99 per leg and run go to --out (default
profiles/unbound/bench_unbound.json), with the HIP-event time of k_r1cs_incidences from a pass of its own."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "keyless-zk-proofs_amd")):
    sys.path.insert(0, p)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def pct(xs, q):
    s = sorted(xs)
    return s[min(len(s) - 1, int(round(q * (len(s) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the circuit (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unbound", "bench_unbound.json"))
    args = ap.parse_args()
    import k16
    import pymodel as pm
    import r1cs_builder as rb
    import unbound_reference as ur
    import valid_key_builder as vkb

    ctx = k16.Context(0)
    L = ctx.L
    shape = ur.large_shape(int(1209229 * args.scale), int(107487 * args.scale), int(26870 * args.scale), seed=17)
    n_wires, rowsA, rowsB, rowsC, _ = rb.from_shape(shape)
    circ = k16.R1cs(ctx, rb.write_from_shape(shape))
    info = circ.info()
    t0 = time.time()
    tmp = tempfile.mkdtemp(prefix="k16_bench_")
    zk = os.path.join(tmp, "key.zkey")
    rng = pm.SplitMix64(2024)
    circ.setup_file(zk, [1 + rng.below(pm.R - 1) for _ in range(5)])
    prover = k16.Prover(ctx, zk)
    os.remove(zk)
    os.rmdir(tmp)
    print("key set up and loaded in %.0f s" % (time.time() - t0), flush=True)
    wtns = [np.ascontiguousarray(vkb.fast_witness(shape, 100 + i)[0], dtype=np.uint8) for i in range(2)]
    n_vars = shape["n_vars"]
    buf = C.create_string_buffer(4096)
    nf, na, nu = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    lst, wires, cls = np.zeros(64, dtype=np.uint32), np.zeros(n_vars, dtype=np.uint32), np.zeros(n_vars, dtype=np.uint8)
    status = np.zeros(n_vars, dtype=np.uint8)

    def chk(rc):
        if rc < 0:
            raise k16.K16Error(rc, (L.k16_last_error(ctx.h) or b"").decode())

    def prove(i):
        chk(L.k16_prover_prove_mem(prover.h, _p(wtns[i]), n_vars, None, None, buf, 4096, None))

    def leg_check(i):
        t = time.perf_counter()
        rc = L.k16_r1cs_check_prover_witness(prover.h, circ.h, C.byref(nf), _p(lst), 64)
        ms = (time.perf_counter() - t) * 1e3
        chk(rc)
        assert nf.value == 0
        return ms

    def leg_scan(i, full=None):
        t = time.perf_counter()
        rc = L.k16_r1cs_unbound_wires(circ.h, C.byref(na), C.byref(nu), _p(wires), _p(cls), n_vars, _p(full))
        ms = (time.perf_counter() - t) * 1e3
        chk(rc)
        return ms

    hip = C.CDLL("libamdhip64.so")
    free0, free1, total = C.c_size_t(), C.c_size_t(), C.c_size_t()
    prove(0)
    leg_check(0)
    hip.hipMemGetInfo(C.byref(free0), C.byref(total))
    first_ms = leg_scan(0, status)
    hip.hipMemGetInfo(C.byref(free1), C.byref(total))
    # the verdict against the reference (not timed)
    t0 = time.time()
    classes = ur.classify(n_wires, rowsA, rowsB, rowsC, rb.witness_ints(wtns[0]))
    want = ur.summary(classes)
    assert status.tolist() == classes and (na.value, nu.value) == want[:2]
    k = want[0] + want[1]
    assert wires[:k].tolist() == want[2] and cls[:k].tolist() == want[3]
    print("first scan %.1f ms; reference agreed in %.0f s" % (first_ms, time.time() - t0), flush=True)
    n_pairs = circ.incidences()
    n_walked = n_pairs - circ.wire_constraints(0, cap=0)[0]        # wire 0's column is not on the device
    counts = {"bound": classes.count(ur.BOUND), "absent": want[0], "unbound": want[1]}
    out = {"gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "n_wires": n_vars, "n_constraints": info["n_constraints"],
           "n_terms": info["n_terms"], "incidences": n_pairs, "incidences_walked": n_walked,
           "scan_device_bytes": free0.value - free1.value,
           "scan_device_bytes_per_incidence_walked": (free0.value - free1.value) / max(n_walked, 1), "classes": counts,
           "first_call_ms": first_ms, "calls_per_leg_per_run": args.calls, "warmup_per_leg": args.warmup,
           "legs": {"check": "k16_r1cs_check_prover_witness", "scan": "k16_r1cs_unbound_wires (list of all free wires, no status map)"},
           "runs": []}
    legs = [("check", leg_check), ("scan", leg_scan)]
    for i in range(args.warmup):
        for _, fn in legs:
            fn(0)
    for run in range(args.runs):
        prove(run % len(wtns))
        t = {name: [] for name, _ in legs}
        for i in range(args.calls):
            for name, fn in legs:
                t[name].append(fn(0))
        row = {name: {"p50_ms": statistics.median(t[name]), "p99_ms": pct(t[name], 0.99), "min_ms": min(t[name])} for name, _ in legs}
        out["runs"].append(row)
        print("run %d  " % run + "   ".join("%s p50 %.3f p99 %.3f ms" % (name, row[name]["p50_ms"], row[name]["p99_ms"]) for name, _ in legs), flush=True)
    out["p50_of_runs_ms"] = {name: statistics.median(r[name]["p50_ms"] for r in out["runs"]) for name, _ in legs}
    out["scan_over_check_p50"] = out["p50_of_runs_ms"]["scan"] / out["p50_of_runs_ms"]["check"]
    ctx.stats_enable(True)
    ctx.stats_reset()
    for i in range(args.calls):
        leg_scan(0)
    n_l, ms = ctx.stats_get("r1cs_incidences")
    out["kernel_us"] = {"r1cs_incidences": {"launches": n_l, "mean_us": ms * 1e3 / max(n_l, 1)}}
    ctx.stats_enable(False)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    circ.close()
    prover.close()
    ctx.close()


if __name__ == "__main__":
    main()
