"""The wide classes of the open-set solve (k16_r1cs_open_system_ex with max_wires 128 / 256) beside the 64-wire call, same
process, same check, alternating call by call -- the method of tools/bench_open_system.py.
    python tools/bench_open_wide.py [--runs 5] [--calls 20] [--warmup 3] [--decompositions 4096] [--scale 1.0] [--circuits LIST] [--out FILE.json]
Circuits:
    generated   section 10f's circuit (tools/bench_complete_bits.py): --decompositions gadgets of 64 bits, each feeding two linear
                constraints; fixed = what the closure with rules = 1 (the PIN rule) does not leave OPEN.  Legs: the cap at 64, 128
                and 256, and the closure with rules = 3 beside them
    chains      64 open chains each of 64, 128 and 256 wires, one circuit per size (rank n - 1 a component): the 64-wire
                circuit runs k_r1cs_open_rref<64> -- the unchanged kernel, the yardstick -- through the cap 64, the other two the
                wide kernel through the cap 256.  Reported per pivot: call p50 / (n - 1) and kernel time / (n - 1).  One
                direction call on a chain of each size
    sparse      64 components each of 256 wires whose reduced form stays sparse: row j is a_j x_j + x_(j+1) + b_j x_(j+2) = s for
                even j and c_j x_(j+1) = s for odd j (every odd wire pinned alone), so a new pivot's column lies in at most two
                basis rows -- the case the per-row masks of the wide kernel are for, where a chain is the case they cannot help
    keyless     the SYNTHETIC circuit of the Keyless shape with the seed of DESIGN.md section 10d: its components have at most
                four wires, so the cap changes nothing: outputs compared, 256 against 64 timed
Per leg: the p50 of the run p50s, the lowest and highest run p50, the largest p99; from HIP events in a pass of their own the
upload and the kernel per size class (scopes r1cs_open_upload, r1cs_open_rref16 / 32 / 64 / 128 / 256).  Output: --out (default
profiles/open_wide/bench_open_wide.json)."""
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

SCOPES = ("r1cs_open_upload", "r1cs_open_rref16", "r1cs_open_rref32", "r1cs_open_rref64", "r1cs_open_rref128", "r1cs_open_rref256")


def pct(xs, q):
    s = sorted(xs)
    return s[min(len(s) - 1, int(round(q * (len(s) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--decompositions", type=int, default=4096)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the Keyless-shape circuit (rehearsals)")
    ap.add_argument("--circuits", default="chains,generated,keyless")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_wide", "bench_open_wide.json"))
    args = ap.parse_args()
    import determined_bits_reference as db
    import k16
    import open_system_reference as osr
    import r1cs_builder as rb
    import unbound_reference as ur
    import valid_key_builder as vkb

    ctx = k16.Context(0)
    L, vp = ctx.L, lambda a: a.ctypes.data_as(C.c_void_p)

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def alternate(name, legs):
        """legs: [(label, fn)], alternating call by call; returns the per-leg summary"""
        for _ in range(args.warmup):
            for _, fn in legs:
                fn()
        runs = []
        for run in range(args.runs):
            t = {n_: [] for n_, _ in legs}
            for _ in range(args.calls):
                for n_, fn in legs:
                    t[n_].append(timed(fn))
            runs.append({n_: {"p50_ms": statistics.median(t[n_]), "p99_ms": pct(t[n_], 0.99)} for n_, _ in legs})
            print("%s run %d  " % (name, run) + "   ".join("%s p50 %.3f" % (n_, runs[-1][n_]["p50_ms"]) for n_, _ in legs), flush=True)
        return {n_: {"p50_of_runs_ms": statistics.median(r[n_]["p50_ms"] for r in runs), "lowest_run_p50_ms": min(r[n_]["p50_ms"] for r in runs),
                     "highest_run_p50_ms": max(r[n_]["p50_ms"] for r in runs), "largest_p99_ms": max(r[n_]["p99_ms"] for r in runs)} for n_, _ in legs}

    def device(fn):
        """HIP events, a pass of its own: ms per call per scope"""
        ctx.stats_enable(True)
        ctx.stats_reset()
        for _ in range(args.calls):
            fn()
        out = {}
        for scope in SCOPES:
            n_l, ms = ctx.stats_get(scope)
            if n_l:
                out[scope] = {"launches": n_l, "ms_per_call": ms / args.calls}
        ctx.stats_enable(False)
        return out

    n64 = [C.c_uint64() for _ in range(8)]
    lst, lst_cls = np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint8)

    def leg_open(circ, fixed, max_wires):
        if max_wires is None:
            return lambda: ctx._chk(L.k16_r1cs_open_system(circ.h, vp(fixed), *(C.byref(x) for x in n64[:7]), vp(lst), vp(lst_cls), 64, None, None))
        return lambda: ctx._chk(L.k16_r1cs_open_system_ex(circ.h, vp(fixed), max_wires, *(C.byref(x) for x in n64[:7]), vp(lst), vp(lst_cls), 64, None, None))

    def counts_of(res):
        return {k: res[k] for k in ("n_forced", "n_free", "n_undecided", "n_skipped", "n_absent", "n_components", "n_dims")}

    def share(res):
        outside = res["n_forced"] + res["n_free"] + res["n_undecided"] + res["n_skipped"]
        return res["n_skipped"] / outside if outside else 0.0

    out = {"gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "calls_per_leg_per_run": args.calls, "runs": args.runs, "warmup_per_leg": args.warmup}
    which = args.circuits.split(",")

    if "chains" in which:
        per = {}
        circs = {}
        for n in (64, 128, 256):
            w = osr.values(1 + 64 * n, 31)
            cons, at = [], 1
            for _ in range(64):                                             # an open chain: rank n - 1
                cons += [osr.linear([(at + j, 1 + j % 3), (at + j + 1, 1)], w) for j in range(n - 1)]
                at += n
            circuit = osr.circuit_of(len(w), cons)
            circ = k16.R1cs(ctx, rb.write(*circuit, n_prv_in=0))
            assert circ.check(np.ascontiguousarray(rb.witness_bytes(w), dtype=np.uint8).reshape(-1))[0] == 0
            fixed = np.zeros(len(w), dtype=np.uint8)
            fixed[0] = 1
            res = circ.open_system(fixed, max_wires=256 if n > 64 else 64)
            assert res["n_free"] == 64 * n and res["n_dims"] == 64 and res["n_skipped"] == 0, res
            circs[n] = (circ, fixed)
        legs = [("chains_%d" % n, leg_open(circs[n][0], circs[n][1], 256 if n > 64 else 64)) for n in (64, 128, 256)]
        summary = alternate("chains", legs)
        for n in (64, 128, 256):
            circ, fixed = circs[n]
            dev = device(legs[(64, 128, 256).index(n)][1])
            kernel = dev.get("r1cs_open_rref%d" % n, {}).get("ms_per_call", 0.0)
            got = {}
            ms = [timed(lambda: got.update(circ.open_direction(fixed, 1 + n // 2, max_wires=256 if n > 64 else 64))) for _ in range(5)]
            assert got["rank"] == n - 1 and len(got["d"]) == n
            per[str(n)] = dict(summary["chains_%d" % n], components=64, pivots_per_component=n - 1, device_ms_of_a_call=dev,
                               call_ms_per_pivot=summary["chains_%d" % n]["p50_of_runs_ms"] / (n - 1), kernel_ms_per_pivot=kernel / (n - 1),
                               direction_call_p50_ms=statistics.median(ms), direction_non_zeros=len(got["d"]))
            circ.close()
        out["chains"] = {"circuit": "64 open chains each of n wires, one circuit per n; n = 64 through the cap 64 (k_r1cs_open_rref<64>), 128 and 256 "
                                    "through the cap 256 (k_r1cs_open_rref_wide)", "by_wires": per}

    if "sparse" in which:
        n = 256
        w = osr.values(1 + 64 * n, 33)
        cons, at = [], 1
        for _ in range(64):
            for j in range(0, n - 2, 2):
                cons.append(osr.linear([(at + j, 2 + j % 5), (at + j + 1, 1), (at + j + 2, 3 + j % 7)], w))
                cons.append(osr.linear([(at + j + 1, 5 + j % 3)], w))
            at += n
        circuit = osr.circuit_of(len(w), cons)
        circ = k16.R1cs(ctx, rb.write(*circuit, n_prv_in=0))
        assert circ.check(np.ascontiguousarray(rb.witness_bytes(w), dtype=np.uint8).reshape(-1))[0] == 0
        fixed = np.zeros(len(w), dtype=np.uint8)
        fixed[0] = 1
        res = circ.open_system(fixed, want_maps=True, max_wires=256)
        sizes = np.unique(res["comp"][res["comp"] != k16.OPEN_NO_COMPONENT], return_counts=True)[1]
        got = circ.open_direction(fixed, 1, max_wires=256)
        leg = leg_open(circ, fixed, 256)
        summary = alternate("sparse", [("sparse_256", leg)])
        dev = device(leg)
        out["sparse"] = dict(summary["sparse_256"], circuit="64 components of 256 wires, three-wire rows on the even wires and every odd wire pinned alone",
                             classes=counts_of(res), component_wires=sorted(set(sizes.tolist())), rank=got["rank"], rows=got["comp_rows"],
                             device_ms_of_a_call=dev, kernel_ms_per_pivot=dev.get("r1cs_open_rref256", {}).get("ms_per_call", 0.0) / max(1, got["rank"]))
        circ.close()

    if "generated" in which:
        circuit, w, _, seed_list = db.generated(args.decompositions, 64)
        circ = k16.R1cs(ctx, rb.write(*circuit))
        assert circ.check(np.ascontiguousarray(rb.witness_bytes(w), dtype=np.uint8).reshape(-1))[0] == 0
        status = circ.determined_wires(seed_list, cap=0, want_maps=True, rules=k16.DET_RULE_PIN)[5]
        fixed = np.ascontiguousarray(status != k16.DET_OPEN, dtype=np.uint8)
        by_cap = {}
        for cap in (64, 128, 256):
            res = circ.open_system(fixed, want_maps=True, max_wires=cap)
            comp = res["comp"][res["comp"] != k16.OPEN_NO_COMPONENT]
            sizes, n_of = np.unique(np.unique(comp, return_counts=True)[1], return_counts=True)
            by_cap[str(cap)] = {"classes": counts_of(res), "skipped_share_of_outside_wires": share(res),
                                "components_by_size": {str(int(a)): int(b) for a, b in zip(sizes, n_of)}}
            if cap == 256:
                at = np.nonzero((res["status"] >= k16.OPEN_FORCED) & (res["status"] <= k16.OPEN_UNDECIDED))[0]
                by_cap["256"]["a_component"] = {k: v for k, v in circ.open_direction(fixed, int(at[0]), max_wires=256).items() if k != "d"} if at.size else None
        rules3 = circ.determined_wires(seed_list, cap=0, want_maps=True, rules=k16.DET_RULE_PIN | k16.DET_RULE_BITS)
        seed = np.array(seed_list, dtype=np.uint32)
        n32 = C.c_uint32()

        def leg_closure(rules):
            return lambda: ctx._chk(L.k16_r1cs_determined_wires_ex(circ.h, vp(seed), len(seed), rules, C.byref(n64[0]), C.byref(n64[1]), C.byref(n64[2]),
                                                                    C.byref(n32), vp(lst), 64, None, None, None, C.byref(n64[3]), None))

        legs = [("open_system", leg_open(circ, fixed, None))] + [("open_system_ex_%d" % cap, leg_open(circ, fixed, cap)) for cap in (64, 128, 256)] + \
               [("closure_rules_1", leg_closure(k16.DET_RULE_PIN)), ("closure_rules_3", leg_closure(k16.DET_RULE_PIN | k16.DET_RULE_BITS))]
        summary = alternate("generated", legs)
        out["generated"] = {"circuit": "%d decompositions of 64 bits, each feeding two linear constraints; fixed: what the closure with rules = 1 does not leave OPEN"
                                       % args.decompositions, "n_wires": circuit[0], "n_constraints": len(circuit[1]), "by_max_wires": by_cap,
                            "closure_rules_3": {"n_derived": int(rules3[0]), "n_absent": int(rules3[1]), "n_open": int(rules3[2])}, "legs": summary,
                            "device_ms_of_a_call": {str(cap): device(leg_open(circ, fixed, cap)) for cap in (64, 128, 256)}}
        circ.close()

    if "keyless" in which:
        shape = ur.large_shape(int(1209229 * args.scale), int(107487 * args.scale), int(26870 * args.scale), seed=17)
        seed_list = [s for s in range(1, shape["prod0"]) if s % 97]
        full = np.ascontiguousarray(vkb.fast_witness(shape, 100)[0], dtype=np.uint8).reshape(-1)
        circ = k16.R1cs(ctx, rb.write_from_shape(shape))
        assert circ.check(full)[0] == 0
        status = circ.determined_wires(seed_list, cap=0, want_maps=True, rules=k16.DET_RULE_PIN)[5]
        fixed = np.ascontiguousarray(status != k16.DET_OPEN, dtype=np.uint8)
        a, b = circ.open_system(fixed, want_maps=True, max_wires=64), circ.open_system(fixed, want_maps=True, max_wires=256)
        same = all((a[k] == b[k]).all() if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)
        assert same
        summary = alternate("keyless", [("open_system_ex_64", leg_open(circ, fixed, 64)), ("open_system_ex_256", leg_open(circ, fixed, 256))])
        lo, hi = summary["open_system_ex_64"]["lowest_run_p50_ms"], summary["open_system_ex_64"]["highest_run_p50_ms"]
        out["keyless"] = {"circuit": "synthetic circuit of the Keyless shape (tests/valid_key_builder.py), not the real one; seed: the bit and byte wires "
                                     "without every 97th", "classes": counts_of(a), "outputs_identical": bool(same), "legs": summary,
                          "difference_256_minus_64_ms": summary["open_system_ex_256"]["p50_of_runs_ms"] - summary["open_system_ex_64"]["p50_of_runs_ms"],
                          "spread_of_the_64_leg_ms": hi - lo}
        circ.close()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
