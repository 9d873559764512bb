"""The open-set solve (k16_r1cs_open_system) beside the closure whose OPEN wires it reads, same process, same check, alternating
call by call -- the method of tools/bench_determined.py.
    python tools/bench_open_system.py [--runs 5] [--calls 20] [--warmup 3] [--decompositions 4096] [--scale 1.0] [--circuits LIST] [--verify] [--out FILE.json]
Three circuits:
    keyless     the SYNTHETIC circuit of the Keyless shape with the seed of DESIGN.md section 10d (the bit and byte wires without
                every 97th)
    generated   section 10f's circuit (tools/bench_complete_bits.py): --decompositions gadgets of 64 bits, each feeding two linear
                constraints; seed = its givens.  The closure runs with rules = 1, so the decompositions stay OPEN: components of
                more than 64 wires, which the solve SKIPS -- the report says how many
    mixed       64 open chains each of 16, 32 and 64 wires, seed wire 0: the one circuit here that reaches the kernels of the two
                larger size classes (rank n - 1, so n - 1 inversions a component)
Per circuit: the closure (k16_r1cs_determined_wires_ex, rules = 1, with the status map) gives fixed = status != DET_OPEN; then the
legs closure (cap 64, no maps) and open_system (cap 64, no maps) alternate.  Reported: the classes, the histogram of component
sizes, the share of the outside wires that is SKIPPED, the p50 of the run p50s and the largest p99 per leg, and -- from HIP events
in a pass of their own -- the upload (scope r1cs_open_upload) and the kernel per size class (r1cs_open_rref16 / 32 / 64); what
remains of a call is the host's: verdict download, kinds, components, work list, class bytes back, counts.  One
k16_r1cs_open_direction call per class of wire found is timed as well.  --verify compares every count and map with the
big-integer reference of tests/open_system_reference.py (minutes on the large circuits).  Output: --out (default
profiles/open_system/bench_open_system.json)."""
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

BUCKETS = [(1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, 32), (33, 64), (65, 1 << 32)]


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
    ap.add_argument("--circuits", default="keyless,generated,mixed", help="comma-separated: keyless, generated, mixed")
    ap.add_argument("--verify", action="store_true", help="compare with the big-integer reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_system", "bench_open_system.json"))
    args = ap.parse_args()
    import determined_bits_reference as db
    import k16
    import open_system_reference as osr
    import r1cs_builder as rb
    import unbound_reference as ur
    import valid_key_builder as vkb

    ctx = k16.Context(0)

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def bench(name, circuit, r1cs_bytes, wtns, seed_list, note):
        n_wires, M = circuit[0], len(circuit[1])
        circ = k16.R1cs(ctx, r1cs_bytes)
        assert circ.check(wtns)[0] == 0
        status = circ.determined_wires(seed_list, cap=0, want_maps=True, rules=k16.DET_RULE_PIN)[5]
        fixed = np.ascontiguousarray(status != k16.DET_OPEN, dtype=np.uint8)
        first_ms = timed(lambda: circ.open_system(fixed, cap=64))
        res = circ.open_system(fixed, want_maps=True)
        counts = {k: res[k] for k in ("n_forced", "n_free", "n_undecided", "n_skipped", "n_absent", "n_components", "n_dims")}
        outside = res["n_forced"] + res["n_free"] + res["n_undecided"] + res["n_skipped"]
        assert outside + res["n_absent"] + int(fixed.sum()) == n_wires and (res["status"][fixed != 0] == k16.OPEN_FIXED).all()
        comp = res["comp"][res["comp"] != k16.OPEN_NO_COMPONENT]
        sizes = np.unique(comp, return_counts=True)[1] if comp.size else np.zeros(0, dtype=np.int64)
        assert sizes.size == res["n_components"] and int(sizes[sizes > k16.OPEN_MAX_WIRES].sum()) == res["n_skipped"]
        hist = {("%d" % lo if lo == hi else "%d+" % lo if hi > 1 << 31 else "%d-%d" % (lo, hi)): int(((sizes >= lo) & (sizes <= hi)).sum())
                for lo, hi in BUCKETS}
        if args.verify:
            t0 = time.time()
            want = osr.analyse(circuit, rb.witness_ints(wtns.reshape(-1, 32)), np.nonzero(fixed)[0].tolist())
            assert counts == {k: want[k] for k in counts}, (name, counts)
            assert res["status"].tolist() == want["classes"] and res["comp"].tolist() == want["comp"]
            for x in [s for s, k in enumerate(want["classes"]) if k == osr.FREE][:32]:
                assert circ.open_direction(fixed, x)["d"] == osr.direction(want, x), (name, x)
            print("%s: the reference agreed in %.0f s" % (name, time.time() - t0), flush=True)
        print("%s: %s; components by size %s; first call %.1f ms" % (name, counts, hist, first_ms), flush=True)
        # the timed legs go through ctypes directly: no list or mask is rebuilt per call
        L, vp = ctx.L, lambda a: a.ctypes.data_as(C.c_void_p)
        seed = np.array(seed_list, dtype=np.uint32)
        n64 = [C.c_uint64() for _ in range(8)]
        n32, lst, lst_cls = C.c_uint32(), np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint8)

        def leg_closure():
            ctx._chk(L.k16_r1cs_determined_wires_ex(circ.h, vp(seed), len(seed), k16.DET_RULE_PIN, C.byref(n64[0]), C.byref(n64[1]),
                                                    C.byref(n64[2]), C.byref(n32), vp(lst), 64, None, None, None, C.byref(n64[3]), None))

        def leg_open():
            ctx._chk(L.k16_r1cs_open_system(circ.h, vp(fixed), *(C.byref(x) for x in n64[:7]), vp(lst), vp(lst_cls), 64, None, None))

        legs = [("closure", leg_closure), ("open_system", leg_open)]
        for _ in range(args.warmup):
            for _, fn in legs:
                fn()
        runs = []
        for run in range(args.runs):
            t = {n_: [] for n_, _ in legs}
            for _ in range(args.calls):
                for n_, fn in legs:
                    t[n_].append(timed(fn))
            row = {n_: {"p50_ms": statistics.median(t[n_]), "p99_ms": pct(t[n_], 0.99), "min_ms": min(t[n_])} for n_, _ in legs}
            runs.append(row)
            print("%s run %d  " % (name, run) + "   ".join("%s p50 %.3f p99 %.3f ms" % (n_, row[n_]["p50_ms"], row[n_]["p99_ms"]) for n_, _ in legs), flush=True)
        p50 = {n_: statistics.median(r[n_]["p50_ms"] for r in runs) for n_, _ in legs}
        ctx.stats_enable(True)
        ctx.stats_reset()
        for _ in range(args.calls):
            legs[1][1]()
        device = {}
        for scope in ("r1cs_open_upload", "r1cs_open_rref16", "r1cs_open_rref32", "r1cs_open_rref64"):
            n_l, ms = ctx.stats_get(scope)
            if n_l:
                device[scope] = {"launches": n_l, "ms_per_call": ms / args.calls}
        ctx.stats_enable(False)
        on_device = sum(v["ms_per_call"] for v in device.values())
        directions = {}
        for k, label in ((k16.OPEN_FREE, "free"), (k16.OPEN_FORCED, "forced"), (k16.OPEN_UNDECIDED, "undecided"), (k16.OPEN_SKIPPED, "skipped")):
            at = np.nonzero(res["status"] == k)[0]
            if at.size:
                x = int(at[at.size // 2])
                got = {}
                ms = [timed(lambda: got.update(circ.open_direction(fixed, x))) for _ in range(5)]
                directions[label] = {"wire": x, "comp_wires": got["comp_wires"], "comp_rows": got["comp_rows"], "rank": got["rank"],
                                     "non_zeros": len(got["d"]), "p50_ms": statistics.median(ms)}
        out = {"circuit": note, "n_wires": n_wires, "n_constraints": M, "incidences": circ.incidences(), "n_seed": len(seed_list),
               "n_fixed": int(fixed.sum()), "outside_wires_in_terms": outside, "classes": counts, "components_by_size": hist,
               "skipped_share_of_outside_wires": res["n_skipped"] / outside if outside else 0.0, "first_call_ms": first_ms,
               "p50_of_runs_ms": p50, "largest_p99_ms": {n_: max(r[n_]["p99_ms"] for r in runs) for n_, _ in legs},
               "open_system_over_closure": p50["open_system"] / p50["closure"], "device_ms_of_an_open_system_call": device,
               "host_and_downloads_ms_of_an_open_system_call": p50["open_system"] - on_device, "direction_calls": directions, "runs": runs}
        circ.close()
        return out

    out = {"gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "calls_per_leg_per_run": args.calls, "warmup_per_leg": args.warmup,
           "legs": {"closure": "k16_r1cs_determined_wires_ex, rules = 1, cap 64, no maps", "open_system": "k16_r1cs_open_system, cap 64, no maps"}}
    which = args.circuits.split(",")
    if "mixed" in which:                                                # every size class of the kernel, which the other two do not reach
        sizes = [n for n in (16, 32, 64) for _ in range(64)]
        w = osr.values(1 + sum(sizes), 31)
        cons, at = [], 1
        for n in sizes:                                                 # an open chain: rank n - 1, n - 1 inversions a component
            cons += [osr.linear([(at + j, 1 + j % 3), (at + j + 1, 1)], w) for j in range(n - 1)]
            at += n
        circuit = osr.circuit_of(len(w), cons)
        out["mixed"] = bench("mixed", circuit, rb.write(*circuit, n_prv_in=0), np.ascontiguousarray(rb.witness_bytes(w), dtype=np.uint8).reshape(-1),
                             [0], "64 open chains each of 16, 32 and 64 wires: 192 components, every wire FREE; seed: wire 0")
    shape = ur.large_shape(int(1209229 * args.scale), int(107487 * args.scale), int(26870 * args.scale), seed=17)
    if "keyless" in which:
        n_wires, rowsA, rowsB, rowsC, _ = rb.from_shape(shape)
        seed_list = [s for s in range(1, shape["prod0"]) if s % 97]
        full = np.ascontiguousarray(vkb.fast_witness(shape, 100)[0], dtype=np.uint8).reshape(-1)
        out["keyless"] = bench("keyless", (n_wires, rowsA, rowsB, rowsC), rb.write_from_shape(shape), full, seed_list,
                               "synthetic circuit of the Keyless shape (tests/valid_key_builder.py), not the real one; seed: the bit and "
                               "byte wires without every 97th")
    if "generated" in which:
        circuit, w, _, seed_list = db.generated(args.decompositions, 64)
        out["generated"] = bench("generated", circuit, rb.write(*circuit), np.ascontiguousarray(rb.witness_bytes(w), dtype=np.uint8).reshape(-1), seed_list,
                                 "%d decompositions of 64 bits, each feeding two linear constraints; closure with rules = 1" % args.decompositions)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "runs"} if isinstance(v, dict) and "runs" in v else v) for k, v in out.items()}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
