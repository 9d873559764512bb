"""The second-value scan (k16_r1cs_second_values) beside the unbound-wire scan (k16_r1cs_unbound_wires) and the check whose sums
both read (k16_r1cs_check_prover_witness), same process, alternating call by call.
    python tools/bench_second_values.py [--runs 5] [--calls 50] [--warmup 5] [--scale 1.0] [--out FILE.json]
Circuit: the SYNTHETIC circuit of the Keyless shape, made and sized as tools/bench_unbound.py makes it.  Its bit wires sit in
their own bit row and in few product rows, so most of them are two-valued: these timings and class counts are the synthetic
circuit's, not the real circuit's.  Recorded:
    first        the first k16_r1cs_second_values of a fresh object: the incidence list is built and uploaded, the per-wire
                 buffers are made, then the scan
    check        k16_r1cs_check_prover_witness before each round of scans -- the witness of the last prove, read in place
    unbound      k16_r1cs_unbound_wires, list of all free wires, no status map
    second_64    k16_r1cs_second_values with cap 64: both walks, the masks' download, the host's pass, 64 shifts
    second_all   the same with every two-valued wire listed and its shift downloaded (one inversion per listed wire)
with the device bytes the scan added on top of the unbound-wire scan's, the wires per class and every count, list and shift
asserted against the big-integer reference of tests/second_value_reference.py.  Every call is timed around its C entry point and
ends in a device synchronise of its own; per leg the p50 of the run p50s and the largest p99 go to --out (default
profiles/second_values/bench_second_values.json), with the kernels' HIP-event times from a pass of their own."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "second_values", "bench_second_values.json"))
    args = ap.parse_args()
    import k16
    import pymodel as pm
    import r1cs_builder as rb
    import second_value_reference as sv
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
    nf, na, nu, n2 = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    lst, wires, cls = np.zeros(64, dtype=np.uint32), np.zeros(n_vars, dtype=np.uint32), np.zeros(n_vars, dtype=np.uint8)
    two, shifts = np.zeros(n_vars, dtype=np.uint32), np.zeros((n_vars, 32), dtype=np.uint8)
    status = np.zeros(n_vars, dtype=np.uint8)

    def chk(rc):
        if rc < 0:
            raise k16.K16Error(rc, (L.k16_last_error(ctx.h) or b"").decode())

    def prove(i):
        chk(L.k16_prover_prove_mem(prover.h, _p(wtns[i]), n_vars, None, None, buf, 4096, None))

    def timed(call):
        t = time.perf_counter()
        rc = call()
        ms = (time.perf_counter() - t) * 1e3
        chk(rc)
        return ms

    def leg_check():
        ms = timed(lambda: L.k16_r1cs_check_prover_witness(prover.h, circ.h, C.byref(nf), _p(lst), 64))
        assert nf.value == 0
        return ms

    def leg_unbound():
        return timed(lambda: L.k16_r1cs_unbound_wires(circ.h, C.byref(na), C.byref(nu), _p(wires), _p(cls), n_vars, None))

    def leg_second(cap, full=None):
        return timed(lambda: L.k16_r1cs_second_values(circ.h, C.byref(n2), _p(two), _p(shifts), cap, _p(full)))

    hip = C.CDLL("libamdhip64.so")
    total = C.c_size_t()

    def free_bytes():
        f = C.c_size_t()
        hip.hipMemGetInfo(C.byref(f), C.byref(total))
        return f.value

    prove(0)
    leg_check()
    before = free_bytes()
    first_ms = leg_second(n_vars, status)
    first_bytes = before - free_bytes()
    # what the unbound-wire scan alone allocates: a second object that runs only that scan; the difference is this scan's own
    other = k16.R1cs(ctx, rb.write_from_shape(shape))
    chk(L.k16_r1cs_check_prover_witness(prover.h, other.h, C.byref(nf), _p(lst), 64))
    before = free_bytes()
    chk(L.k16_r1cs_unbound_wires(other.h, C.byref(na), C.byref(nu), None, None, 0, None))
    unbound_bytes = before - free_bytes()
    other.close()
    # the verdict against the reference (not timed)
    t0 = time.time()
    classes, want_shifts = sv.classify(n_wires, rowsA, rowsB, rowsC, rb.witness_ints(wtns[0]))
    want_n, want_wires, want_d = sv.summary(classes, want_shifts)
    assert status.tolist() == classes and n2.value == want_n
    assert two[:want_n].tolist() == want_wires
    assert shifts[:want_n].tobytes() == b"".join(d.to_bytes(32, "little") for d in want_d)
    leg_unbound()
    unbound = ur.summary([ur.BOUND if k == sv.TWO_VALUED else k for k in classes])
    k = unbound[0] + unbound[1]
    assert (na.value, nu.value) == unbound[:2] and wires[:k].tolist() == unbound[2] and cls[:k].tolist() == unbound[3]
    print("first scan %.1f ms; reference agreed in %.0f s" % (first_ms, time.time() - t0), flush=True)
    n_pairs = circ.incidences()
    n_walked = n_pairs - circ.wire_constraints(0, cap=0)[0]        # wire 0's column is not on the device
    counts = {"single": classes.count(ur.BOUND), "absent": unbound[0], "unbound": unbound[1], "two_valued": want_n}
    out = {"circuit": "synthetic circuit of the Keyless shape (tests/valid_key_builder.py), not the real one",
           "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "n_wires": n_vars, "n_constraints": info["n_constraints"],
           "n_terms": info["n_terms"], "incidences": n_pairs, "incidences_walked": n_walked,
           "device_bytes_first_call": first_bytes, "device_bytes_unbound_scan_alone": unbound_bytes,
           "device_bytes_second_values_own": first_bytes - unbound_bytes, "classes": counts,
           "first_call_ms": first_ms, "calls_per_leg_per_run": args.calls, "warmup_per_leg": args.warmup,
           "legs": {"check": "k16_r1cs_check_prover_witness", "unbound": "k16_r1cs_unbound_wires (list of all free wires, no status map)",
                    "second_64": "k16_r1cs_second_values, cap 64, wires and shifts, no status map",
                    "second_all": "k16_r1cs_second_values, every two-valued wire and its shift, no status map"},
           "runs": []}
    legs = [("check", leg_check), ("unbound", leg_unbound), ("second_64", lambda: leg_second(64)), ("second_all", lambda: leg_second(n_vars))]
    for i in range(args.warmup):
        for _, fn in legs:
            fn()
    for run in range(args.runs):
        prove(run % len(wtns))
        t = {name: [] for name, _ in legs}
        for i in range(args.calls):
            for name, fn in legs:
                t[name].append(fn())
        row = {name: {"p50_ms": statistics.median(t[name]), "p99_ms": pct(t[name], 0.99), "min_ms": min(t[name])} for name, _ in legs}
        out["runs"].append(row)
        print("run %d  " % run + "   ".join("%s p50 %.3f p99 %.3f ms" % (name, row[name]["p50_ms"], row[name]["p99_ms"]) for name, _ in legs), flush=True)
    out["p50_of_runs_ms"] = {name: statistics.median(r[name]["p50_ms"] for r in out["runs"]) for name, _ in legs}
    out["largest_p99_ms"] = {name: max(r[name]["p99_ms"] for r in out["runs"]) for name, _ in legs}
    p50 = out["p50_of_runs_ms"]
    out["multiples_p50"] = {leg: {"of_check": p50[leg] / p50["check"], "of_unbound": p50[leg] / p50["unbound"]} for leg in ("second_64", "second_all")}
    ctx.stats_enable(True)
    out["kernel_us"] = {}
    for leg, fn in legs[1:]:
        ctx.stats_reset()
        for i in range(args.calls):
            fn()
        out["kernel_us"][leg] = {}
        for name in ("r1cs_incidences", "r1cs_kinds", "r1cs_agree", "r1cs_shifts"):
            n_l, ms = ctx.stats_get(name)
            if n_l:
                out["kernel_us"][leg][name] = {"launches": n_l, "mean_us": ms * 1e3 / n_l}
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
