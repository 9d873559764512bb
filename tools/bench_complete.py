"""The witness completion (k16_r1cs_complete_witness) beside the two calls it stands in for on a witness somebody else
computed -- the check (k16_r1cs_check_mem) and the determinism closure (k16_r1cs_determined_wires, 64 OPEN wires listed) -- same
process, same witness, alternating call by call.
    python tools/bench_complete.py [--runs 5] [--calls 30] [--warmup 3] [--scale 1.0] [--depth 10000] [--out FILE.json]
Circuit: the SYNTHETIC circuit of the Keyless shape, made and sized as tools/bench_determined.py makes it, with that tool's
seed as the givens: the recipe's own inputs -- the bit and byte wires -- without every 97th of them, which stands for a hint
nobody supplied; the product wires are left to the completion.  Class counts and depth are this recipe's and these givens', not
the real circuit's.  Recorded:
    first     the first completion of a fresh object: incidence list, closure buffers and row view are built and uploaded
    check     k16_r1cs_check_mem of the full witness
    closure   k16_r1cs_determined_wires, cap 64, no maps, on that check
    complete  k16_r1cs_complete_witness, cap 64 and cap_failed 64, no maps, from the same bytes
with the comparison of record, complete against check + closure, n_rounds, the four class counts and every count, list, map
and returned byte of one call asserted against the big-integer reference of tests/solve_reference.py.
SPLIT of a completion: the kernels' HIP-event times from a pass of their own, grouped as rounds (r1cs_det_init,
r1cs_solve_mask, _derive, _commit, r1cs_det_expand) and closing check (r1cs_rows, r1cs_judge, r1cs_solve_close); upload and
download as the wall time of a copy of the witness's size each way from the same pageable buffer; the rest of the call's p50 is
host work and the synchronise per round.
DEPTH LEG: a chain x_i+1 = x_i x_i + 1 of --depth constraints, one wire per round, completed from x_1 and compared with the
chain's witness.  Every call is timed around its C entry point and ends in a device synchronise of its own; per leg the p50 of
the run p50s and the largest p99 go to --out (default profiles/complete/bench_complete.json)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
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
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the circuit (rehearsals)")
    ap.add_argument("--depth", type=int, default=10000, help="constraints of the chain of the depth leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complete", "bench_complete.json"))
    args = ap.parse_args()
    import determined_reference as dr
    import k16
    import r1cs_builder as rb
    import solve_reference as sr
    import unbound_reference as ur
    import valid_key_builder as vkb

    ctx = k16.Context(0)
    L = ctx.L
    shape = ur.large_shape(int(1209229 * args.scale), int(107487 * args.scale), int(26870 * args.scale), seed=17)
    n_wires, rowsA, rowsB, rowsC, _ = rb.from_shape(shape)
    circuit = (n_wires, rowsA, rowsB, rowsC)
    given_list = [s for s in range(1, shape["prod0"]) if s % 97]
    given = np.array(given_list, dtype=np.uint32)
    circ = k16.R1cs(ctx, rb.write_from_shape(shape))
    info = circ.info()
    M = info["n_constraints"]
    full = np.ascontiguousarray(vkb.fast_witness(shape, 100)[0], dtype=np.uint8)
    entry = full.copy()
    work = entry.copy()
    nf, noc, ns, nab, no, nd = (C.c_uint64(0) for _ in range(6))
    nr = C.c_uint32(0)
    failed, opened = np.zeros(max(M, 64), dtype=np.uint32), np.zeros(n_wires, dtype=np.uint32)
    status, rounds, by = np.zeros(n_wires, dtype=np.uint8), np.zeros(n_wires, dtype=np.uint32), np.zeros(n_wires, dtype=np.uint32)

    def chk(rc):
        if rc < 0:
            raise k16.K16Error(rc, (L.k16_last_error(ctx.h) or b"").decode())

    def timed(call):
        t = time.perf_counter()
        rc = call()
        ms = (time.perf_counter() - t) * 1e3
        chk(rc)
        return ms

    def leg_check():
        ms = timed(lambda: L.k16_r1cs_check_mem(ctx.h, circ.h, _p(full), n_wires, C.byref(nf), _p(failed), 64))
        assert nf.value == 0
        return ms

    def leg_closure():
        return timed(lambda: L.k16_r1cs_determined_wires(circ.h, _p(given), len(given), C.byref(nd), C.byref(nab), C.byref(no), C.byref(nr),
                                                         _p(opened), 64, None, None, None))

    def complete(h, wt, gv, n_gv, cap, cap_failed, maps):
        return timed(lambda: L.k16_r1cs_complete_witness(h, _p(wt), _p(gv), n_gv, C.byref(ns), C.byref(nab), C.byref(no), C.byref(nr),
                                                         C.byref(nf), _p(failed), cap_failed, C.byref(noc), _p(opened), cap,
                                                         *((_p(status), _p(rounds), _p(by)) if maps else (None, None, None))))

    def leg_complete():
        np.copyto(work, entry)
        return complete(circ.h, work, given, len(given), 64, 64, False)

    first_ms = complete(circ.h, work, given, len(given), n_wires, M, True)
    # the verdict against the reference (not timed)
    t0 = time.time()
    want = sr.complete(circuit, rb.witness_ints(full), given_list)
    counts = sr.summary(want)
    assert (ns.value, nab.value, no.value, nr.value, nf.value, noc.value) == counts, ((ns.value, nab.value, no.value, nr.value, nf.value, noc.value), counts)
    assert opened[:counts[2]].tolist() == sr.open_wires(want) and failed[:counts[4]].tolist() == want["failed"]
    assert status.tolist() == want["status"] and rounds.tolist() == want["round"] and by.tolist() == want["by"]
    assert work.tobytes() == rb.witness_bytes(want["wtns"]).tobytes()
    print("first completion %.1f ms, %d rounds; reference agreed in %.0f s" % (first_ms, counts[3], time.time() - t0), flush=True)
    out = {"circuit": "synthetic circuit of the Keyless shape (tests/valid_key_builder.py), not the real one",
           "givens": "the bit and byte wires 1 .. prod0 - 1 without every 97th (%d wires), given as a list" % len(given_list),
           "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "n_wires": n_wires, "n_constraints": M, "n_terms": info["n_terms"],
           "incidences": circ.incidences(), "n_rounds": counts[3],
           "classes": {"given": want["status"].count(sr.GIVEN), "solved": counts[0], "absent": counts[1], "open": counts[2]},
           "n_failed": counts[4], "n_open_constraints": counts[5],
           "wires_per_round": [want["round"].count(k) for k in range(1, counts[3] + 1)],
           "first_call_ms": first_ms, "calls_per_leg_per_run": args.calls, "warmup_per_leg": args.warmup,
           "legs": {"check": "k16_r1cs_check_mem, cap 64", "closure": "k16_r1cs_determined_wires, cap 64, no maps",
                    "complete": "k16_r1cs_complete_witness, cap 64, cap_failed 64, no maps (the copy of the entry bytes is outside the timer)"},
           "runs": []}
    legs = [("check", leg_check), ("closure", leg_closure), ("complete", leg_complete)]
    for i in range(args.warmup):
        for _, fn in legs:
            fn()
    for run in range(args.runs):
        t = {name: [] for name, _ in legs}
        for i in range(args.calls):
            for name, fn in legs:
                t[name].append(fn())
        row = {name: {"p50_ms": statistics.median(t[name]), "p99_ms": pct(t[name], 0.99), "min_ms": min(t[name])} for name, _ in legs}
        out["runs"].append(row)
        print("run %d  " % run + "   ".join("%s p50 %.3f p99 %.3f ms" % (name, row[name]["p50_ms"], row[name]["p99_ms"]) for name, _ in legs), flush=True)
    p50 = out["p50_of_runs_ms"] = {name: statistics.median(r[name]["p50_ms"] for r in out["runs"]) for name, _ in legs}
    out["largest_p99_ms"] = {name: max(r[name]["p99_ms"] for r in out["runs"]) for name, _ in legs}
    out["complete_over_check_plus_closure"] = p50["complete"] / (p50["check"] + p50["closure"])
    # the split: kernels by HIP events, the two copies by a copy of the same size each way
    ctx.stats_enable(True)
    ctx.stats_reset()
    for i in range(args.calls):
        leg_complete()
    groups = {"rounds": ("r1cs_det_init", "r1cs_solve_mask", "r1cs_solve_derive", "r1cs_solve_commit", "r1cs_det_expand"),
              "closing_check": ("r1cs_rows", "r1cs_judge", "r1cs_solve_close")}
    out["kernel_us"], split = {}, {}
    for group, names in groups.items():
        split[group + "_kernels_ms"] = 0.0
        for name in names:
            n_l, ms = ctx.stats_get(name)
            if n_l:
                out["kernel_us"][name] = {"launches": n_l, "mean_us": ms * 1e3 / n_l, "us_per_call": ms * 1e3 / args.calls}
                split[group + "_kernels_ms"] += ms / args.calls
    ctx.stats_enable(False)
    dbuf = ctx.alloc(full.nbytes)
    up, down = [], []
    for i in range(max(args.calls // 3, 5)):
        t = time.perf_counter()
        dbuf.upload(work)
        up.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        chk(L.k16_d2h(ctx.h, _p(work), dbuf.ptr, work.nbytes))
        down.append((time.perf_counter() - t) * 1e3)
    dbuf.free()
    split["upload_ms"], split["download_ms"] = statistics.median(up), statistics.median(down)
    split["host_and_synchronises_ms"] = p50["complete"] - sum(split.values())
    out["split_of_complete_p50_ms"] = split
    circ.close()

    # ---- the depth leg
    chain, w, header, _ = dr.chain(args.depth)
    deep = k16.R1cs(ctx, rb.write(*chain, n_pub_out=header[0], n_pub_in=header[1], n_prv_in=header[2]))
    n = chain[0]
    d_entry = np.full((n, 32), 0xFF, dtype=np.uint8)
    d_entry[:2] = rb.witness_bytes(w[:2])
    d_work = d_entry.copy()

    def deep_call():
        np.copyto(d_work, d_entry)
        return complete(deep.h, d_work, None, 0, 0, 0, False)

    deep_first = deep_call()
    assert (ns.value, nab.value, no.value, nr.value, nf.value, noc.value) == (args.depth, 0, 0, args.depth, 0, 0)
    assert d_work.tobytes() == rb.witness_bytes(w).tobytes()
    deep_ms = [deep_call() for _ in range(5)]
    deep.close()
    out["depth_leg"] = {"circuit": "chain x_i+1 = x_i x_i + 1, completed from x_1", "constraints": args.depth, "n_wires": n,
                        "n_rounds": args.depth, "first_call_ms": deep_first, "calls_ms": deep_ms, "p50_ms": statistics.median(deep_ms),
                        "ms_per_round": statistics.median(deep_ms) / args.depth}
    print("depth leg: %d rounds in %.1f ms, %.4f ms a round" % (args.depth, out["depth_leg"]["p50_ms"], out["depth_leg"]["ms_per_round"]), flush=True)
    print(json.dumps({k: v for k, v in out.items() if k not in ("runs", "wires_per_round")}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
