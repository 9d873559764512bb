"""Verified proving (k16_prover_prove_mem_verified) against the two-call way, same process, alternating proof by proof.
    python tools/bench_prove_verified.py [--runs 8] [--proofs 100] [--warmup 10] [--legs a,b,c] [--out FILE.json]
Key: the valid Keyless-shape key tools/config4_wave.py builds (nVars 1,343,588, N = 2^21, one public input).  Legs:
    a  k16_prover_prove_mem
    b  k16_prover_prove_mem, then k16_verify_batch of that proof's bytes: the two calls are timed and added; turning the JSON
       into bytes stays outside the timed region (an integrator that has out_proof does not do it at all)
    c  k16_prover_prove_mem_verified
Every call is timed around its C entry point on prepared arrays and ends in a device synchronise of its own.  The legs
alternate proof by proof (a, b, c, a, b, c, ...), so that whatever else the box does hits all three alike; a run is
--proofs proofs per leg; p50 and p99 per leg and per run go to --out together with the process's GPU_MAX_HW_QUEUES.  Every
proof's flag is asserted.  --pkg DIR takes k16.py and libk16.so from DIR (an older build, legs a and b only): the same
tool on the same box says whether leg a moved.  --quick: one short run (for a kernel trace under rocprofv3)."""
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


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def pct(xs, q):
    s = sorted(xs)
    return s[min(len(s) - 1, int(round(q * (len(s) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--proofs", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the circuit (rehearsals)")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "keyless-zk-proofs_amd"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if args.quick:
        args.runs, args.proofs, args.warmup = 1, 10, 3
    legs = args.legs.split(",")
    pkg = os.path.abspath(args.pkg)
    if pkg != os.path.join(ROOT, "keyless-zk-proofs_amd"):
        os.environ["K16_LIB_PATH"] = os.path.join(pkg, "libk16.so")
    for p in (os.path.join(ROOT, "tests"), pkg):
        sys.path.insert(0, p)
    import k16
    import groth16_io as gio
    import valid_key_builder as vkb

    ctx = k16.Context(0)
    L = ctx.L
    key = vkb.build(lambda g, sc: ctx.synth_points_scalars(g, sc), int(1209229 * args.scale), int(107487 * args.scale),
                    int(26870 * args.scale), seed=17)
    tmp = tempfile.mkdtemp(prefix="k16_bench_")
    zk = os.path.join(tmp, "key.zkey")
    with open(zk, "wb") as f:
        f.write(key["zkey"])
    key["zkey"] = None
    prover = k16.Prover(ctx, zk)
    V = k16.VerifyingKey.from_zkey(ctx, zk) if "c" in legs else k16.VerifyingKey(ctx, key["vk"])
    os.remove(zk)
    os.rmdir(tmp)
    if "c" in legs:
        prover.set_vk(V)
    wits = [vkb.fast_witness(key["shape"], 100 + i) for i in range(4)]
    wtns = [np.ascontiguousarray(w[0], dtype=np.uint8) for w in wits]
    inps = [np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in w[1]), dtype=np.uint8).copy() for w in wits]
    n_vars = key["n_vars"]
    buf = C.create_string_buffer(4096)
    proof = np.zeros(256, dtype=np.uint8)
    ok8 = np.zeros(1, dtype=np.uint8)
    okc = C.c_uint8(0)

    def chk(rc):
        if rc < 0:
            raise k16.K16Error(rc, (L.k16_last_error(ctx.h) or b"").decode())

    def leg_a(i):
        t0 = time.perf_counter()
        rc = L.k16_prover_prove_mem(prover.h, _p(wtns[i]), n_vars, None, None, buf, 4096, None)
        ms = (time.perf_counter() - t0) * 1e3
        chk(rc)
        return ms

    def leg_b(i):
        ms = leg_a(i)
        pr = np.frombuffer(gio.proof_from_json(buf.value.decode()), dtype=np.uint8).copy()      # (not timed)
        t0 = time.perf_counter()
        rc = L.k16_verify_batch(ctx.h, V.h, _p(pr), _p(inps[i]), 1, _p(ok8))
        ms += (time.perf_counter() - t0) * 1e3
        chk(rc)
        assert ok8[0] == 1
        return ms

    def leg_c(i):
        okc.value = 0
        t0 = time.perf_counter()
        rc = L.k16_prover_prove_mem_verified(prover.h, _p(wtns[i]), n_vars, None, None, buf, 4096, None, _p(proof), C.byref(okc))
        ms = (time.perf_counter() - t0) * 1e3
        chk(rc)
        assert okc.value == 1
        return ms

    fn = {"a": leg_a, "b": leg_b, "c": leg_c}
    for k in range(args.warmup):
        for leg in legs:
            fn[leg](k % len(wtns))
    out = {"gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "n_vars": n_vars, "domain": key["domain"], "proofs_per_leg_per_run": args.proofs, "warmup_per_leg": args.warmup,
           "legs": {"a": "prove_mem", "b": "prove_mem + verify_batch", "c": "prove_mem_verified"},
           "library": os.path.relpath(pkg, ROOT), "runs": []}
    for run in range(args.runs):
        t = {leg: [] for leg in legs}
        for k in range(args.proofs):
            for leg in legs:
                t[leg].append(fn[leg]((run + k) % len(wtns)))
        row = {leg: {"p50_ms": statistics.median(t[leg]), "p99_ms": pct(t[leg], 0.99), "min_ms": min(t[leg])} for leg in legs}
        if "b" in legs and "c" in legs:
            row["c_below_b"] = row["c"]["p50_ms"] < row["b"]["p50_ms"]
        out["runs"].append(row)
        print("run %d  " % run + "   ".join("%s p50 %.3f p99 %.3f ms" % (leg, row[leg]["p50_ms"], row[leg]["p99_ms"]) for leg in legs), flush=True)
    p50 = {leg: statistics.median(r[leg]["p50_ms"] for r in out["runs"]) for leg in legs}
    out["p50_of_runs_ms"] = p50
    out["p50_spread_ms"] = {leg: [min(r[leg]["p50_ms"] for r in out["runs"]), max(r[leg]["p50_ms"] for r in out["runs"])] for leg in legs}
    if "a" in legs:
        for leg in legs:
            if leg != "a":
                out["%s_minus_a_ms" % leg] = p50[leg] - p50["a"]
    if "b" in legs and "c" in legs:
        out["c_below_b_runs"] = sum(r["c_below_b"] for r in out["runs"])
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    prover.close()
    V.close()
    ctx.close()


if __name__ == "__main__":
    main()
