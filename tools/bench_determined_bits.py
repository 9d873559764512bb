"""The bit rule of the determinism closure (k16_r1cs_determined_wires_ex, K16_DET_RULE_PIN | K16_DET_RULE_BITS) beside the PIN rule
alone, same process, same check, alternating call by call -- the method of tools/bench_determined.py.
    python tools/bench_determined_bits.py [--runs 5] [--calls 20] [--warmup 3] [--decompositions 4096] [--scale 1.0] [--out FILE.json]
Two circuits:
    generated   section 10f's circuit (tools/bench_complete_bits.py): --decompositions gadgets of 64 bits, each feeding two linear
                constraints; seed = its givens.  With the PIN rule alone every bit, y and z are OPEN.
    keyless     the SYNTHETIC circuit of the Keyless shape with the seed of DESIGN.md section 10d (the bit and byte wires without
                every 97th): the report says plainly whether the rule fires on any of its rows, and what a fruitless bit level costs.
Legs, per circuit: closure (k16_r1cs_determined_wires), rules_1 (the new entry point with rules = 1), rules_3 (rules = 3), held
(k16_r1cs_held_wires, no marks); cap 64, no maps.  Every count, list, map and rule byte of one call per rule set is asserted
against the big-integer reference of tests/determined_bits_reference.py, its certificate is replayed, and rules = 1 is compared
byte for byte with the existing call.  The kernels are timed by HIP events in a pass of their own (the scope r1cs_det_bits holds
k_r1cs_bits_filter and k_r1cs_det_bits); on the generated circuit the completion's bit level (scope r1cs_solve_bits) is timed the
same way, in the same process.  Per leg the p50 of the run p50s and the largest p99 go to --out (default
profiles/determined_bits/bench_determined_bits.json)."""
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--decompositions", type=int, default=4096)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the Keyless-shape circuit (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "determined_bits", "bench_determined_bits.json"))
    args = ap.parse_args()
    import determined_bits_reference as db
    import determined_reference as dr
    import k16
    import r1cs_builder as rb
    import unbound_reference as ur
    import valid_key_builder as vkb

    ctx = k16.Context(0)
    L = ctx.L

    def chk(rc):
        if rc < 0:
            raise k16.K16Error(rc, (L.k16_last_error(ctx.h) or b"").decode())

    def bench(name, circuit, r1cs_bytes, wtns, seed_list, note, completion):
        n_wires, M = circuit[0], len(circuit[1])
        circ = k16.R1cs(ctx, r1cs_bytes)
        circ.check(wtns)
        seed = np.array(seed_list, dtype=np.uint32)
        nd, nab, no, nb, nh = (C.c_uint64(0) for _ in range(5))
        nr = C.c_uint32(0)
        opened = np.zeros(n_wires, dtype=np.uint32)
        status, rule = np.zeros(n_wires, dtype=np.uint8), np.zeros(n_wires, dtype=np.uint8)
        rounds, by = np.zeros(n_wires, dtype=np.uint32), np.zeros(n_wires, dtype=np.uint32)

        def call(rules, cap, maps):
            """rules None: the existing entry point"""
            common = (C.byref(nd), C.byref(nab), C.byref(no), C.byref(nr), _p(opened), cap,
                      *((_p(status), _p(rounds), _p(by)) if maps else (None, None, None)))
            t = time.perf_counter()
            if rules is None:
                rc = L.k16_r1cs_determined_wires(circ.h, _p(seed), len(seed), *common)
            else:
                rc = L.k16_r1cs_determined_wires_ex(circ.h, _p(seed), len(seed), rules, *common, C.byref(nb), _p(rule) if maps else None)
            ms = (time.perf_counter() - t) * 1e3
            chk(rc)
            return ms

        def held():
            t = time.perf_counter()
            rc = L.k16_r1cs_held_wires(circ.h, C.byref(nh), None)
            ms = (time.perf_counter() - t) * 1e3
            chk(rc)
            return ms

        res, first_ms = {}, {}
        w_ints = rb.witness_ints(wtns.reshape(-1, 32))
        for rules in (db.PIN, db.PIN | db.BITS):                        # the verdict against the reference (not timed)
            first_ms[rules] = call(rules, n_wires, True)
            t0 = time.time()
            want = db.closure(circuit, w_ints, seed_list, rules)
            n_derived, n_absent, n_open, n_rounds, n_by_bits, want_open = db.summary(want)
            got = (nd.value, nab.value, no.value, nr.value, nb.value)
            assert got == (n_derived, n_absent, n_open, n_rounds, n_by_bits), (name, rules, got)
            assert opened[:n_open].tolist() == want_open
            assert status.tolist() == want["status"] and rounds.tolist() == want["round"] and by.tolist() == want["by"]
            assert rule.tolist() == want["rule"]
            assert db.replay(circuit, w_ints, seed_list, status.tolist(), rounds.tolist(), by.tolist(), rule.tolist()) is None
            if rules == db.PIN:                                         # ... and the existing call: the same bytes
                keep = [a.copy() for a in (opened, status, rounds, by)]
                call(None, n_wires, True)
                assert (nd.value, nab.value, no.value, nr.value) == got[:4]
                assert all(a.tobytes() == b.tobytes() for a, b in zip(keep, (opened, status, rounds, by)))
            res[rules] = {"n_rounds": n_rounds, "classes": {"seed": want["status"].count(dr.SEED), "derived": n_derived, "absent": n_absent,
                                                            "open": n_open},
                          "n_by_bits": n_by_bits, "wires_per_round": [want["round"].count(k) for k in range(1, n_rounds + 1)],
                          "bit_rounds": sorted({want["round"][s] for s, k in enumerate(want["rule"]) if k == db.BITS})}
            print("%s rules %d: first call %.1f ms, %d rounds, %d by bits, %d open; reference agreed in %.0f s"
                  % (name, rules, first_ms[rules], n_rounds, n_by_bits, n_open, time.time() - t0), flush=True)
        held()
        want_held = db.held_wires(circuit, w_ints)
        assert nh.value == sum(want_held) and circ.held_wires(mark=True)[1].tolist() == want_held
        legs = [("closure", lambda: call(None, 64, False)), ("rules_1", lambda: call(db.PIN, 64, False)),
                ("rules_3", lambda: call(db.PIN | db.BITS, 64, False)), ("held", held)]
        for _ in range(args.warmup):
            for _, fn in legs:
                fn()
        runs = []
        for run in range(args.runs):
            t = {n_: [] for n_, _ in legs}
            for _ in range(args.calls):
                for n_, fn in legs:
                    t[n_].append(fn())
            row = {n_: {"p50_ms": statistics.median(t[n_]), "p99_ms": pct(t[n_], 0.99), "min_ms": min(t[n_])} for n_, _ in legs}
            runs.append(row)
            print("%s run %d  " % (name, run) + "   ".join("%s p50 %.3f p99 %.3f ms" % (n_, row[n_]["p50_ms"], row[n_]["p99_ms"]) for n_, _ in legs), flush=True)
        p50 = {n_: statistics.median(r[n_]["p50_ms"] for r in runs) for n_, _ in legs}

        def kernels(fn, scopes):
            ctx.stats_reset()
            for _ in range(args.calls):
                fn()
            out = {}
            for scope in scopes:
                n_l, ms = ctx.stats_get(scope)
                if n_l:
                    out[scope] = {"launches": n_l, "mean_us": ms * 1e3 / n_l, "us_per_call": ms * 1e3 / args.calls}
            return out

        ctx.stats_enable(True)
        kernel_us = kernels(legs[2][1], ("r1cs_det_init", "r1cs_held", "r1cs_det_derive", "r1cs_det_expand", "r1cs_det_bits"))
        completion_us = None
        if completion:                                                  # the completion's bit level on the same circuit
            entry = np.full((n_wires, 32), 0xFF, dtype=np.uint8)
            full = wtns.reshape(-1, 32)
            for s in [0] + seed_list:
                entry[s] = full[s]
            completion_us = kernels(lambda: circ.complete_witness(entry.reshape(-1), given=seed_list, rules=3, cap=64, cap_failed=64,
                                                                  cap_infeasible=64), ("r1cs_solve_bits",))
        ctx.stats_enable(False)
        out = {"circuit": note, "n_wires": n_wires, "n_constraints": M, "incidences": circ.incidences(), "n_seed": len(seed_list),
               "boolean_wires": circ.boolean_wires(), "held_wires": int(nh.value), "rules_1": res[db.PIN], "rules_3": res[db.PIN | db.BITS],
               "the_rule_fires": res[db.PIN | db.BITS]["n_by_bits"] > 0,
               "first_call_ms": {"rules_1": first_ms[db.PIN], "rules_3": first_ms[db.PIN | db.BITS]},
               "p50_of_runs_ms": p50, "largest_p99_ms": {n_: max(r[n_]["p99_ms"] for r in runs) for n_, _ in legs},
               "rules_3_over_closure": p50["rules_3"] / p50["closure"], "kernel_us_of_a_rules_3_call": kernel_us,
               "kernel_us_of_a_completion_rules_3_call": completion_us, "runs": runs}
        circ.close()
        return out

    out = {"gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "calls_per_leg_per_run": args.calls, "warmup_per_leg": args.warmup,
           "legs": {"closure": "k16_r1cs_determined_wires", "rules_1": "k16_r1cs_determined_wires_ex, rules = 1",
                    "rules_3": "k16_r1cs_determined_wires_ex, rules = 3; all with cap 64, no maps", "held": "k16_r1cs_held_wires, no marks"}}
    circuit, w, _, seed_list = db.generated(args.decompositions, 64)
    out["generated"] = bench("generated", circuit, rb.write(*circuit), np.ascontiguousarray(rb.witness_bytes(w), dtype=np.uint8).reshape(-1), seed_list,
                             "%d decompositions of 64 bits, each feeding two linear constraints" % args.decompositions, True)
    shape = ur.large_shape(int(1209229 * args.scale), int(107487 * args.scale), int(26870 * args.scale), seed=17)
    n_wires, rowsA, rowsB, rowsC, _ = rb.from_shape(shape)
    seed_list = [s for s in range(1, shape["prod0"]) if s % 97]
    full = np.ascontiguousarray(vkb.fast_witness(shape, 100)[0], dtype=np.uint8).reshape(-1)
    out["keyless"] = bench("keyless", (n_wires, rowsA, rowsB, rowsC), rb.write_from_shape(shape), full, seed_list,
                           "synthetic circuit of the Keyless shape (tests/valid_key_builder.py), not the real one; seed: the bit and "
                           "byte wires without every 97th", False)
    print("keyless: the bit rule %s on this circuit" % ("FIRES" if out["keyless"]["the_rule_fires"] else "fires on NO row"), flush=True)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk != "runs"} if isinstance(v, dict) and "runs" in v else v) for k, v in out.items()}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
