"""The bit rule of the witness completion (k16_r1cs_complete_witness_ex, K16_SOLVE_RULE_LINEAR | K16_SOLVE_RULE_BITS) beside the
linear rule alone, same process, same entry bytes, alternating call by call -- the method of tools/bench_complete.py.
    python tools/bench_complete_bits.py [--runs 5] [--calls 20] [--warmup 3] [--decompositions 4096] [--scale 1.0] [--out FILE.json]
Two circuits:
    generated   --decompositions gadgets: x given, its 64 bits b_i (each with its own boolean constraint, in the four forms),
                ONE row sum 2^i b_i = x (orientation, scaling and exponent order vary by gadget), then y = sum a_i b_i and
                z = 3 y + x: two linear constraints behind the bits.  With the linear rule alone every bit, y and z stay OPEN.
    keyless     the SYNTHETIC circuit of the Keyless shape with the givens of tools/bench_complete.py (the closure's seed of
                DESIGN.md section 10d): the report says plainly whether the rule fires on any of its rows.
Legs, per circuit: linear (k16_r1cs_complete_witness), linear_ex (the new entry point with rules = 1), bits (rules = 3); cap 64,
cap_failed 64, cap_infeasible 64, no maps; the copy of the entry bytes is outside the timer.  Every count, list, map and returned
byte of one call per rule set is asserted against the big-integer reference of tests/solve_bits_reference.py, and rules = 1
byte for byte against the existing call.  The bit level's kernels (k_r1cs_bits_filter, k_r1cs_solve_bits, k_r1cs_bits_commit:
the scope r1cs_solve_bits) are timed by HIP events in a pass of their own.  Per leg the p50 of the run p50s and the largest p99
go to --out (default profiles/complete_bits/bench_complete_bits.json)."""
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


def generated(n):
    """(circuit, w, given): n gadgets of 64 bits"""
    import pymodel as pm
    import solve_bits_reference as sb
    R = pm.R
    c = sb.Circuit(0xBE7C)
    for i in range(n):
        x = c.wire(pm.SplitMix64(0x64B175 + i).next(), True)
        bits = c.bits(64, c.w[x])
        exps = list(range(64)) if i % 4 else list(range(63, -1, -1))     # every fourth: the LSB on the highest wire, the second lambda
        value = sum(((c.w[x] >> j) & 1) << e for j, e in enumerate(exps))
        c.w[x] = value
        c.decomposition(bits, exps, x, ("A", "B", "C")[i % 3], 1 if i % 2 else 2 + sb.below(c.rng, R - 2))
        coefs = [1 + (7 * j + i) % 5 for j in range(64)]
        y = c.wire(sum(a * c.w[b] for a, b in zip(coefs, bits)))
        c.rows.mul([(b, a) for a, b in zip(coefs, bits)], [(0, 1)], [(y, 1)])
        z = c.wire(3 * c.w[y] + c.w[x])
        c.rows.mul([(y, 3), (x, 1)], [(0, 1)], [(z, 1)])
    circuit, w, _, given = c.case()
    return circuit, w, given


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--decompositions", type=int, default=4096)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the Keyless-shape circuit (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complete_bits", "bench_complete_bits.json"))
    args = ap.parse_args()
    import k16
    import r1cs_builder as rb
    import solve_bits_reference as sb
    import solve_reference as sr
    import unbound_reference as ur
    import valid_key_builder as vkb

    ctx = k16.Context(0)
    L = ctx.L

    def chk(rc):
        if rc < 0:
            raise k16.K16Error(rc, (L.k16_last_error(ctx.h) or b"").decode())

    def bench(name, circuit, r1cs_bytes, entry, given_list, note):
        n_wires, M = circuit[0], len(circuit[1])
        circ = k16.R1cs(ctx, r1cs_bytes)
        given = np.array(given_list, dtype=np.uint32)
        work = entry.copy()
        ns, nab, no, nf, noc, nb, ni = (C.c_uint64(0) for _ in range(7))
        nr = C.c_uint32(0)
        failed, infeasible, opened = np.zeros(max(M, 64), dtype=np.uint32), np.zeros(max(M, 64), dtype=np.uint32), np.zeros(n_wires, dtype=np.uint32)
        status, rule = np.zeros(n_wires, dtype=np.uint8), np.zeros(n_wires, dtype=np.uint8)
        rounds, by = np.zeros(n_wires, dtype=np.uint32), np.zeros(n_wires, dtype=np.uint32)

        def call(rules, cap, cap_c, maps):
            """rules None: the existing entry point"""
            np.copyto(work, entry)
            common = (C.byref(ns), C.byref(nab), C.byref(no), C.byref(nr), C.byref(nf), _p(failed), cap_c, C.byref(noc), _p(opened), cap,
                      *((_p(status), _p(rounds), _p(by)) if maps else (None, None, None)))
            t = time.perf_counter()
            if rules is None:
                rc = L.k16_r1cs_complete_witness(circ.h, _p(work), _p(given), len(given), *common)
            else:
                rc = L.k16_r1cs_complete_witness_ex(circ.h, _p(work), _p(given), len(given), rules, *common, C.byref(nb), C.byref(ni),
                                                    _p(infeasible), cap_c, _p(rule) if maps else None)
            ms = (time.perf_counter() - t) * 1e3
            chk(rc)
            return ms

        res, first_ms = {}, {}
        w_ints = rb.witness_ints(entry.reshape(-1, 32))
        for rules in (sb.LINEAR, sb.LINEAR | sb.BITS):                  # the verdict against the reference (not timed)
            first_ms[rules] = call(rules, n_wires, M, True)
            t0 = time.time()
            want = sb.complete(circuit, w_ints, given_list, rules)
            counts = sr.summary(want) + (want["n_by_bits"], len(want["infeasible"]))
            got = (ns.value, nab.value, no.value, nr.value, nf.value, noc.value, nb.value, ni.value)
            assert got == counts, (name, rules, got, counts)
            assert opened[:counts[2]].tolist() == sr.open_wires(want) and failed[:counts[4]].tolist() == want["failed"]
            assert infeasible[:counts[7]].tolist() == want["infeasible"]
            assert status.tolist() == want["status"] and rounds.tolist() == want["round"] and by.tolist() == want["by"]
            assert rule.tolist() == want["rule"] and work.tobytes() == rb.witness_bytes(want["wtns"]).tobytes()
            if rules == sb.LINEAR:                                      # ... and the existing call: the same bytes
                keep = [a.copy() for a in (work, failed, opened, status, rounds, by)]
                call(None, n_wires, M, True)
                assert (ns.value, nab.value, no.value, nr.value, nf.value, noc.value) == counts[:6]
                assert all(a.tobytes() == b.tobytes() for a, b in zip(keep, (work, failed, opened, status, rounds, by)))
            res[rules] = {"n_rounds": counts[3], "classes": {"given": want["status"].count(sr.GIVEN), "solved": counts[0], "absent": counts[1],
                                                              "open": counts[2]},
                          "n_failed": counts[4], "n_open_constraints": counts[5], "n_by_bits": counts[6], "n_infeasible": counts[7],
                          "wires_per_round": [want["round"].count(k) for k in range(1, counts[3] + 1)],
                          "bit_rounds": sorted({want["round"][s] for s, k in enumerate(want["rule"]) if k == sb.BITS})}
            print("%s rules %d: first call %.1f ms, %d rounds, %d by bits, %d infeasible; reference agreed in %.0f s"
                  % (name, rules, first_ms[rules], counts[3], counts[6], counts[7], time.time() - t0), flush=True)
        legs = [("linear", lambda: call(None, 64, 64, False)), ("linear_ex", lambda: call(sb.LINEAR, 64, 64, False)),
                ("bits", lambda: call(sb.LINEAR | sb.BITS, 64, 64, False))]
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
        ctx.stats_enable(True)
        ctx.stats_reset()
        for _ in range(args.calls):
            legs[2][1]()
        kernel_us = {}
        for scope in ("r1cs_det_init", "r1cs_solve_mask", "r1cs_solve_derive", "r1cs_solve_commit", "r1cs_det_expand", "r1cs_solve_bits",
                      "r1cs_rows", "r1cs_judge", "r1cs_solve_close"):
            n_l, ms = ctx.stats_get(scope)
            if n_l:
                kernel_us[scope] = {"launches": n_l, "mean_us": ms * 1e3 / n_l, "us_per_call": ms * 1e3 / args.calls}
        ctx.stats_enable(False)
        n_bool = circ.boolean_wires()
        out = {"circuit": note, "n_wires": n_wires, "n_constraints": M, "incidences": circ.incidences(), "n_given": len(given_list),
               "boolean_wires": n_bool, "rules_1": res[sb.LINEAR], "rules_3": res[sb.LINEAR | sb.BITS],
               "the_rule_fires": res[sb.LINEAR | sb.BITS]["n_by_bits"] > 0 or res[sb.LINEAR | sb.BITS]["n_infeasible"] > 0,
               "first_call_ms": {"rules_1": first_ms[sb.LINEAR], "rules_3": first_ms[sb.LINEAR | sb.BITS]},
               "p50_of_runs_ms": p50, "largest_p99_ms": {n_: max(r[n_]["p99_ms"] for r in runs) for n_, _ in legs},
               "bits_over_linear": p50["bits"] / p50["linear"], "kernel_us_of_a_rules_3_call": kernel_us, "runs": runs}
        circ.close()
        return out

    out = {"gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "calls_per_leg_per_run": args.calls, "warmup_per_leg": args.warmup,
           "legs": {"linear": "k16_r1cs_complete_witness", "linear_ex": "k16_r1cs_complete_witness_ex, rules = 1",
                    "bits": "k16_r1cs_complete_witness_ex, rules = 3; all with cap 64, no maps"}}
    circuit, w, given_list = generated(args.decompositions)
    entry = np.full((len(w), 32), 0xFF, dtype=np.uint8)
    wb = rb.witness_bytes(w)
    for s in [0] + given_list:
        entry[s] = wb[s]
    out["generated"] = bench("generated", circuit, rb.write(*circuit), entry.reshape(-1), given_list,
                             "%d decompositions of 64 bits, each feeding two linear constraints" % args.decompositions)
    shape = ur.large_shape(int(1209229 * args.scale), int(107487 * args.scale), int(26870 * args.scale), seed=17)
    n_wires, rowsA, rowsB, rowsC, _ = rb.from_shape(shape)
    given_list = [s for s in range(1, shape["prod0"]) if s % 97]
    full = np.ascontiguousarray(vkb.fast_witness(shape, 100)[0], dtype=np.uint8).reshape(-1)
    out["keyless"] = bench("keyless", (n_wires, rowsA, rowsB, rowsC), rb.write_from_shape(shape), full, given_list,
                           "synthetic circuit of the Keyless shape (tests/valid_key_builder.py), not the real one; givens: the bit and "
                           "byte wires without every 97th")
    print("keyless: the bit rule %s on this circuit" % ("FIRES" if out["keyless"]["the_rule_fires"] else "fires on NO row"), flush=True)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if kk not in ("runs",) and not isinstance(vv, dict) or kk in ("p50_of_runs_ms",)}
                          if isinstance(v, dict) and "runs" in v else v) for k, v in out.items()}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
