"""The determinism closure (k16_r1cs_determined_wires) beside the two scans (k16_r1cs_unbound_wires, k16_r1cs_second_values) and
the check whose sums all three read (k16_r1cs_check_prover_witness), same process, alternating call by call.
    python tools/bench_determined.py [--runs 5] [--calls 50] [--warmup 5] [--scale 1.0] [--depth 10000] [--out FILE.json]
Circuit: the SYNTHETIC circuit of the Keyless shape, made and sized as tools/bench_unbound.py makes it.  Its header calls every
wire an input, so the seed is given as a list: the recipe's own inputs -- the bit and byte wires -- without every 97th of them,
which stands for a hint; the product wires are left to the closure.  Class counts and depth are this recipe's and this seed's,
not the real circuit's.  Recorded:
    first        the first k16_r1cs_determined_wires of a fresh object: the incidence list is built and uploaded, the closure's
                 buffers are made, then the closure
    check        k16_r1cs_check_prover_witness before each round of calls -- the witness of the last prove, read in place
    unbound      k16_r1cs_unbound_wires, list of all free wires, no status map
    second_64    k16_r1cs_second_values with cap 64
    closure_64   k16_r1cs_determined_wires with cap 64, no maps
    closure_all  the same with every OPEN wire listed and status, round and by downloaded
with the device bytes the closure added on top of the incidence list's, n_rounds, the wires per class, the time per round
(closure_64 / n_rounds: initialisation and the final download included) and every count, list and map asserted against the
big-integer reference of tests/determined_reference.py.
DEPTH LEG: a chain x_i+1 = x_i x_i + 1 of --depth constraints, one wire per round; its maps are asserted against what a chain
must give, and its wall time says what the host's synchronise per round costs.
Every call is timed around its C entry point and ends in a device synchronise of its own; per leg the p50 of the run p50s and the
largest p99 go to --out (default profiles/determined/bench_determined.json), with the kernels' HIP-event times from a pass of
their own."""
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
    ap.add_argument("--depth", type=int, default=10000, help="constraints of the chain of the depth leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "determined", "bench_determined.json"))
    args = ap.parse_args()
    import determined_reference as dr
    import k16
    import pymodel as pm
    import r1cs_builder as rb
    import unbound_reference as ur
    import valid_key_builder as vkb

    ctx = k16.Context(0)
    L = ctx.L
    shape = ur.large_shape(int(1209229 * args.scale), int(107487 * args.scale), int(26870 * args.scale), seed=17)
    n_wires, rowsA, rowsB, rowsC, _ = rb.from_shape(shape)
    circuit = (n_wires, rowsA, rowsB, rowsC)
    seed_list = [s for s in range(1, shape["prod0"]) if s % 97]
    seed = np.array(seed_list, dtype=np.uint32)
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
    nd, nab, no, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    lst, wires, cls = np.zeros(64, dtype=np.uint32), np.zeros(n_vars, dtype=np.uint32), np.zeros(n_vars, dtype=np.uint8)
    two, shifts = np.zeros(64, dtype=np.uint32), np.zeros((64, 32), dtype=np.uint8)
    opened, status = np.zeros(n_vars, dtype=np.uint32), np.zeros(n_vars, dtype=np.uint8)
    rounds, by = np.zeros(n_vars, dtype=np.uint32), np.zeros(n_vars, dtype=np.uint32)

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

    def leg_second():
        return timed(lambda: L.k16_r1cs_second_values(circ.h, C.byref(n2), _p(two), _p(shifts), 64, None))

    def closure(h, cap, maps):
        return timed(lambda: L.k16_r1cs_determined_wires(h, _p(seed), len(seed), C.byref(nd), C.byref(nab), C.byref(no), C.byref(nr),
                                                         _p(opened), cap, *((_p(status), _p(rounds), _p(by)) if maps else (None, None, None))))

    hip = C.CDLL("libamdhip64.so")
    total = C.c_size_t()

    def free_bytes():
        f = C.c_size_t()
        hip.hipMemGetInfo(C.byref(f), C.byref(total))
        return f.value

    prove(0)
    leg_check()
    before = free_bytes()
    first_ms = closure(circ.h, n_vars, True)
    first_bytes = before - free_bytes()
    # what the incidence list alone takes: a second object that runs the unbound-wire scan first; the closure's own bytes are what
    # its first call adds there
    other = k16.R1cs(ctx, rb.write_from_shape(shape))
    chk(L.k16_r1cs_check_prover_witness(prover.h, other.h, C.byref(nf), _p(lst), 64))
    chk(L.k16_r1cs_unbound_wires(other.h, C.byref(na), C.byref(nu), None, None, 0, None))
    before = free_bytes()
    closure(other.h, 0, False)
    own_bytes = before - free_bytes()
    other.close()
    # the verdict against the reference (not timed)
    t0 = time.time()
    w_ints = rb.witness_ints(wtns[0])
    want_status, want_rounds, want_by = dr.closure(circuit, w_ints, seed_list)
    n_derived, n_absent, n_open, n_rounds, want_open = dr.summary(want_status, want_rounds)
    assert (nd.value, nab.value, no.value, nr.value) == (n_derived, n_absent, n_open, n_rounds)
    assert opened[:n_open].tolist() == want_open
    assert status.tolist() == want_status and rounds.tolist() == want_rounds and by.tolist() == want_by
    assert dr.replay(circuit, w_ints, seed_list, status.tolist(), rounds.tolist(), by.tolist()) is None
    print("first closure %.1f ms, %d rounds; reference agreed in %.0f s" % (first_ms, n_rounds, time.time() - t0), flush=True)
    n_pairs = circ.incidences()
    out = {"circuit": "synthetic circuit of the Keyless shape (tests/valid_key_builder.py), not the real one",
           "seed": "the bit and byte wires 1 .. prod0 - 1 without every 97th (%d wires), given as a list" % len(seed_list),
           "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "n_wires": n_vars, "n_constraints": info["n_constraints"],
           "n_terms": info["n_terms"], "incidences": n_pairs, "incidences_walked": n_pairs - circ.wire_constraints(0, cap=0)[0],
           "device_bytes_first_call": first_bytes, "device_bytes_closure_own": own_bytes,
           "n_rounds": n_rounds, "classes": {"seed": want_status.count(dr.SEED), "derived": n_derived, "absent": n_absent, "open": n_open},
           "wires_per_round": [want_rounds.count(k) for k in range(1, n_rounds + 1)],
           "first_call_ms": first_ms, "calls_per_leg_per_run": args.calls, "warmup_per_leg": args.warmup,
           "legs": {"check": "k16_r1cs_check_prover_witness", "unbound": "k16_r1cs_unbound_wires (list of all free wires, no status map)",
                    "second_64": "k16_r1cs_second_values, cap 64, wires and shifts, no status map",
                    "closure_64": "k16_r1cs_determined_wires, cap 64, no maps",
                    "closure_all": "k16_r1cs_determined_wires, every OPEN wire, status, round and by downloaded"},
           "runs": []}
    legs = [("check", leg_check), ("unbound", leg_unbound), ("second_64", leg_second),
            ("closure_64", lambda: closure(circ.h, 64, False)), ("closure_all", lambda: closure(circ.h, n_vars, True))]
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
    out["multiples_p50"] = {leg: {"of_check": p50[leg] / p50["check"], "of_unbound": p50[leg] / p50["unbound"]} for leg in ("closure_64", "closure_all")}
    out["ms_per_round_keyless_shape"] = p50["closure_64"] / max(n_rounds, 1)
    ctx.stats_enable(True)
    out["kernel_us"] = {}
    for leg, fn in legs[3:]:
        ctx.stats_reset()
        for i in range(args.calls):
            fn()
        out["kernel_us"][leg] = {}
        for name in ("r1cs_det_init", "r1cs_det_derive", "r1cs_det_expand"):
            n_l, ms = ctx.stats_get(name)
            if n_l:
                out["kernel_us"][leg][name] = {"launches": n_l, "mean_us": ms * 1e3 / n_l, "us_per_call": ms * 1e3 / args.calls}
    ctx.stats_enable(False)
    circ.close()
    prover.close()

    # ---- the depth leg
    chain, w, header, _ = dr.chain(args.depth)
    deep = k16.R1cs(ctx, rb.write(*chain, n_pub_out=header[0], n_pub_in=header[1], n_prv_in=header[2]))
    assert deep.check(rb.witness_bytes(w))[0] == 0
    n = chain[0]
    d_status, d_rounds, d_by = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)

    def deep_call():
        return timed(lambda: L.k16_r1cs_determined_wires(deep.h, None, 0, C.byref(nd), C.byref(nab), C.byref(no), C.byref(nr),
                                                         None, 0, _p(d_status), _p(d_rounds), _p(d_by)))

    deep_first = deep_call()
    assert (nd.value, nab.value, no.value, nr.value) == (args.depth, 0, 0, args.depth)
    assert d_rounds.tolist() == [0, 0] + list(range(1, args.depth + 1)) and d_by.tolist() == [dr.NONE, dr.NONE] + list(range(args.depth))
    assert d_status.tolist() == [dr.SEED, dr.SEED] + [dr.DERIVED] * args.depth
    deep_ms = [deep_call() for _ in range(5)]
    deep.close()
    out["depth_leg"] = {"circuit": "chain x_i+1 = x_i x_i + 1", "constraints": args.depth, "n_wires": n, "n_rounds": args.depth,
                        "first_call_ms": deep_first, "calls_ms": deep_ms, "p50_ms": statistics.median(deep_ms),
                        "ms_per_round": statistics.median(deep_ms) / args.depth}
    out["depth_10000_from_keyless_per_round_ms"] = out["ms_per_round_keyless_shape"] * 10000
    print("depth leg: %d rounds in %.1f ms, %.4f ms a round" % (args.depth, out["depth_leg"]["p50_ms"], out["depth_leg"]["ms_per_round"]), flush=True)
    print(json.dumps({k: v for k, v in out.items() if k not in ("runs", "wires_per_round")}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
